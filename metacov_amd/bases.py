"""Per-position base counts: what the reads say at each position.

    with BaseCounter(n_ref) as bc:
        bc.begin(tids, starts, ends, min_baseq=15)
        bc.add_bam("x.bam")                  # or add_reads(...) batch by batch
        planes = bc.counts()                 # uint32 [6, N]: A, C, G, T, N, DEL
        sites = bc.sites(min_depth=10, min_count=2, min_ppm=10000)
        cons = bc.consensus(min_depth=10, min_count=2, call_ppm=500000)
        write_fasta(fh, "contig_1", cons.compact(0))   # the letters were called on the device

    a, c, g, t = count_coverage("x.bam", "contig_1", 0, 1000)
    letters, summary = consensus("x.bam", "contig_1")

The pileup runs on the GPU (csrc/bases.hip, mc_bases_* in
include/metacov_amd.h); the records come from the host source in
csrc/bases_src.cpp (decode="host", the default: file decode on host threads
bounds the path end to end) or from the GPU decoder's bases mode
(decode="gpu", GpuBaseSource: the records stay in device memory between
decode and pileup).  These are the numbers of pysam's `AlignmentFile.count_coverage()`,
`samtools mpileup`, pysamstats and bam-readcount; the reference has no
counterpart.  The contract (CIGAR walk, channels, quality rule, segments,
sites, the consensus rule, insertion alleles) is the header's.  Insertions
are opt-in: begin(..., insertions=True) collects the I ops' alleles beside the
planes, insertions() returns their grouped table and consensus(...,
insertions=True) writes the called ones into the compact letters.  Strand is
opt-in too: begin(..., strand=True) keeps the counts of the reverse-strand
reads (flag & 0x10) beside the totals (counts_reverse(); forward = counts() -
counts_reverse()), and sites(..., min_alt_strand=K) asks for an alternative
allele seen K times on each strand.  So are the quality sums: begin(...,
quality=True) keeps, per channel, the sum of the counted bases' quality bytes
and of their reads' MAPQ (quality() -> (bq, mq)); the reads then come with
their mapq column, and sites(..., min_alt_baseq=Q, min_alt_mapq=Q) asks for an
alternative allele whose mean qualities reach the thresholds.  Two counters
begun on the same segments compare their samples: a.compare(b, window=500)
reduces both counters' planes on the device to per-window conANI / popANI
between the samples and the distance of their allele frequencies
(Comparison; compare(path_a, path_b, contig) is the one-call form).
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check, ptr

CHANNELS = ("A", "C", "G", "T", "N", "DEL")
A, C, G, T, N, DEL = range(6)
FLAG_FILTER = 0x704
GET_CHUNK = 1 << 22                 # positions per mc_bases_get of write_all


def contig_names(references):
    """The contig id of each header name: its first word, or the name itself
    where it has no word."""
    return [w.split()[0] if w.split() else w for w in references]


def dims(lib=None):
    """Tile positions of the pileup kernel."""
    lib = lib or _lib.load()
    t = ctypes.c_int32()
    check(lib.mc_bases_dims(ctypes.byref(t)), lib)
    return t.value


def quality_dims(lib=None):
    """(positions per workgroup of the quality pileup kernel, reads it walks
    between two flushes of its packed LDS cells)."""
    lib = lib or _lib.load()
    a, b = ctypes.c_int32(), ctypes.c_int32()
    check(lib.mc_bases_quality_dims(ctypes.byref(a), ctypes.byref(b)), lib)
    return a.value, b.value


def ins_dims(lib=None):
    """(events one workgroup sorts in LDS, longest callable insertion)."""
    lib = lib or _lib.load()
    a, b = ctypes.c_int32(), ctypes.c_int32()
    check(lib.mc_bases_ins_dims(ctypes.byref(a), ctypes.byref(b)), lib)
    return a.value, b.value


class Sites:
    """Sites of S segments, in segment order: segment s owns rows
    first[s] .. first[s + 1]; pos [n] int64 relative to the contig, ascending
    within a segment; counts [n, 6] uint32 (A, C, G, T, N, DEL); rev_counts
    [n, 6] uint32, the reverse-strand reads' share of counts, on a counter
    that tracks strand, else None; bq_sums and mq_sums [n, 6] uint32, the
    sites' quality and MAPQ sums, on a counter that tracks quality, else
    None."""

    def __init__(self, first, pos, counts, rev_counts=None, bq_sums=None, mq_sums=None):
        self.first = np.asarray(first, np.int64)
        self.pos = np.asarray(pos, np.int64)
        self.counts = np.asarray(counts, np.uint32).reshape(-1, 6)
        self.rev_counts = None if rev_counts is None else np.asarray(rev_counts, np.uint32).reshape(-1, 6)
        self.bq_sums = None if bq_sums is None else np.asarray(bq_sums, np.uint32).reshape(-1, 6)
        self.mq_sums = None if mq_sums is None else np.asarray(mq_sums, np.uint32).reshape(-1, 6)

    def __len__(self):
        return len(self.pos)


CONS_IUPAC, CONS_FILL_REF, CONS_INS = 1, 2, 4    # MC_CONS_*
MAX_INS_LEN = 32                    # a longer insertion is OTHER


class Insertions:
    """The allele table of S segments (BaseCounter.insertions): segment s owns
    rows first[s] .. first[s + 1], sorted by (index, other, length, code) and
    unique.  index [n] int64 plane index of the anchor (the position before
    the inserted bases), length [n] int32 and code [n] uint64 (base j of the
    allele is (code >> 2 * (length - 1 - j)) & 3, A C G T = 0..3), other [n]
    uint8 (1: the position's row of insertions longer than MAX_INS_LEN or with
    an ambiguity code; length 0, code 0), count [n] uint32."""

    def __init__(self, first, index, length, code, other, count):
        self.first = np.asarray(first, np.int64)
        self.index = np.asarray(index, np.int64)
        self.length = np.asarray(length, np.int32)
        self.code = np.asarray(code, np.uint64)
        self.other = np.asarray(other, np.uint8)
        self.count = np.asarray(count, np.uint32)

    def __len__(self):
        return len(self.index)

    def sequence(self, k):
        """Row k's inserted bases as a str; '*' for an OTHER row."""
        if self.other[k]:
            return "*"
        n, c = int(self.length[k]), int(self.code[k])
        return "".join("ACGT"[(c >> (2 * (n - 1 - j))) & 3] for j in range(n))
CONS_COLS = 8
# the summary's columns
POSITIONS, CALLED, AMBIGUOUS, NOCALL, LOW, DELETED, DIFFERS, LENGTH = range(8)
SUMMARY_COLUMNS = ("positions", "called", "ambiguous", "nocall", "low", "deleted", "differs", "length")


class Consensus:
    """The consensus of S segments (BaseCounter.consensus), valid until the
    counter's next consensus, add_*, set_counts or begin.  first [S + 1]:
    segment s owns compact letters first[s] .. first[s + 1]; summary [S, 8]
    int64 (columns POSITIONS .. LENGTH); n: compact letters in all.  The
    letters stay on the device; aligned(s) and compact(s) fetch one segment's
    as uint8 ASCII, GET_CHUNK at a time.  inserted: None, or with
    insertions=True int64 [S, 2]: insertions called, bases inserted (the
    compact letters and the summary's length then include them)."""

    def __init__(self, counter, seg_off, first, summary, n, inserted=None):
        self._bc = counter
        self.inserted = None if inserted is None else np.asarray(inserted, np.int64).reshape(-1, 2)
        self.seg_off = np.asarray(seg_off, np.int64)
        self.first = np.asarray(first, np.int64)
        self.summary = np.asarray(summary, np.int64).reshape(-1, CONS_COLS)
        self.n = int(n)

    def __len__(self):
        return len(self.first) - 1

    def aligned(self, s):
        """One letter per position of segment s, '-' where it is deleted."""
        return self._bc.consensus_letters(False, int(self.seg_off[s]), int(self.seg_off[s + 1] - self.seg_off[s]))

    def compact(self, s):
        """Segment s's letters without the deleted positions."""
        return self._bc.consensus_letters(True, int(self.first[s]), int(self.first[s + 1] - self.first[s]))


DIV_COLS = 8                        # MC_DIV_COLS
DIV_MIN_WINDOW = 16                 # MC_DIV_MIN_WINDOW
DIV_COLUMNS = ("positions", "covered", "bases", "snv", "pi_fix", "compared", "con_diff", "pop_diff")
PI_ONE = 4294967296.0               # pi_fix is 32.32 fixed point


def _ratio(num, den):
    """num / den as float64, NaN where den is 0."""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    out = np.full(num.shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


class _WindowRows:
    """What Diversity and Comparison share: segment s owns rows win_first[s] ..
    win_first[s + 1], its windows in order; rows [n, 8] int64 with the class's
    COLUMNS, each also an attribute; window: the window length asked for (0:
    whole segments).  Both have the columns compared, con_diff and pop_diff."""
    COLUMNS = ()

    def __init__(self, win_first, rows, window=0):
        self.win_first = np.asarray(win_first, np.int64)
        self.rows = np.asarray(rows, np.int64).reshape(-1, len(self.COLUMNS))
        self.window = int(window)
        for c, name in enumerate(self.COLUMNS):
            setattr(self, name, self.rows[:, c])

    def __len__(self):
        return len(self.rows)

    def segment(self):
        """int64 [n]: the segment of each row."""
        return np.repeat(np.arange(len(self.win_first) - 1, dtype=np.int64), np.diff(self.win_first))

    def start(self):
        """int64 [n]: each window's first position, counted from its segment's start."""
        k = np.arange(len(self.rows), dtype=np.int64) - self.win_first[:-1][self.segment()]
        return k * self.window

    def end(self):
        return self.start() + self.positions

    def con_ani(self):
        return 1.0 - _ratio(self.con_diff, self.compared)

    def pop_ani(self):
        return 1.0 - _ratio(self.pop_diff, self.compared)


class Diversity(_WindowRows):
    """The diversity rows of S segments (BaseCounter.diversity): segment s owns
    rows win_first[s] .. win_first[s + 1], its windows in order; rows [n, 8]
    int64 with the columns DIV_COLUMNS, each also an attribute (positions,
    covered, bases, snv, pi_fix, compared, con_diff, pop_diff).  window: the
    window length asked for (0: whole segments).  The ratio methods return
    float64 with NaN where the denominator is 0."""
    COLUMNS = DIV_COLUMNS

    def pi(self):
        """Nucleotide diversity: the mean over the covered positions."""
        return _ratio(self.pi_fix / PI_ONE, self.covered)

    def breadth(self):
        return _ratio(self.covered, self.positions)

    def mean_depth(self):
        """Mean A + C + G + T over all the window's positions."""
        return _ratio(self.bases, self.positions)

    def snv_density(self):
        return _ratio(self.snv, self.covered)


CMP_COLS = 8                        # MC_CMP_COLS
CMP_COLUMNS = ("positions", "covered_a", "covered_b", "compared", "con_diff", "pop_diff", "snv", "dist_fix")


class Comparison(_WindowRows):
    """The comparison rows of two samples over S segments
    (BaseCounter.compare): segment s owns rows win_first[s] .. win_first[s + 1],
    its windows in order; rows [n, 8] int64 with the columns CMP_COLUMNS, each
    also an attribute (positions, covered_a, covered_b, compared, con_diff,
    pop_diff, snv, dist_fix).  window: the window length asked for (0: whole
    segments).  The ratio methods return float64 with NaN where the
    denominator is 0."""
    COLUMNS = CMP_COLUMNS

    def breadth_a(self):
        return _ratio(self.covered_a, self.positions)

    def breadth_b(self):
        return _ratio(self.covered_b, self.positions)

    def overlap(self):
        """The share of the window's positions covered in both samples."""
        return _ratio(self.compared, self.positions)

    def distance(self):
        """The mean total-variation distance of the two samples' allele
        frequencies over the compared positions."""
        return _ratio(self.dist_fix / PI_ONE, self.compared)


class BaseSource:
    """One mc_bases_src: the kept records of a coordinate-sorted BAM."""

    def __init__(self, path, n_threads=0, flag_filter=FLAG_FILTER, min_mapq=0, lib=None):
        self._lib = lib or _lib.load()
        self._h = ctypes.c_void_p()
        check(self._lib.mc_bases_src_open(str(path).encode(), int(n_threads), int(flag_filter), int(min_mapq),
                                          ctypes.byref(self._h)), self._lib)
        n = ctypes.c_int32()
        check(self._lib.mc_bases_src_n_targets(self._h, ctypes.byref(n)), self._lib)
        self.references, self.lengths = [], []
        for i in range(n.value):
            name, length = ctypes.c_char_p(), ctypes.c_int64()
            check(self._lib.mc_bases_src_target(self._h, i, ctypes.byref(name), ctypes.byref(length)), self._lib)
            self.references.append(name.value.decode())
            self.lengths.append(length.value)

    def next(self, max_reads=1 << 20, max_bases=1 << 27):
        """The next batch as a dict of numpy views (valid until the next call),
        in mc_bases_add_batch's layout; None at the end of the file."""
        n = ctypes.c_int64()
        check(self._lib.mc_bases_src_next(self._h, int(max_reads), int(max_bases), ctypes.byref(n)), self._lib)
        n = n.value
        self._n = n
        if n == 0:
            return None
        p = [ctypes.c_void_p() for _ in range(9)]
        check(self._lib.mc_bases_src_batch(self._h, *[ctypes.byref(x) for x in p]), self._lib)

        def view(q, dtype, count):
            if count == 0:
                return np.zeros(0, dtype)
            buf = (ctypes.c_char * (count * np.dtype(dtype).itemsize)).from_address(q.value)
            return np.frombuffer(buf, dtype=dtype, count=count)

        cig_off = view(p[2], np.int64, n + 1)
        seq_off = view(p[5], np.int64, n + 1)
        qual_off = view(p[7], np.int64, n + 1)
        return {"tid": view(p[0], np.int32, n), "pos": view(p[1], np.int32, n), "cig_off": cig_off,
                "cigar": view(p[3], np.uint32, int(cig_off[n])), "l_seq": view(p[4], np.int32, n),
                "seq_off": seq_off, "seq": view(p[6], np.uint8, int(seq_off[n])),
                "qual_off": qual_off, "qual": view(p[8], np.uint8, int(qual_off[n]))}

    def flags(self):
        """uint16 [n]: the BAM flag words of the last batch next() returned (a
        view, valid until the next call); the strand is flag & 0x10."""
        n = getattr(self, "_n", 0)
        if n == 0:
            return np.zeros(0, np.uint16)
        p = ctypes.c_void_p()
        check(self._lib.mc_bases_src_flags(self._h, ctypes.byref(p)), self._lib)
        buf = (ctypes.c_char * (2 * n)).from_address(p.value)
        return np.frombuffer(buf, dtype=np.uint16, count=n)

    def mapq(self):
        """uint8 [n]: the MAPQ bytes of the last batch next() returned (a view,
        valid until the next call)."""
        n = getattr(self, "_n", 0)
        if n == 0:
            return np.zeros(0, np.uint8)
        p = ctypes.c_void_p()
        check(self._lib.mc_bases_src_mapq(self._h, ctypes.byref(p)), self._lib)
        buf = (ctypes.c_char * n).from_address(p.value)
        return np.frombuffer(buf, dtype=np.uint8, count=n)

    def counts(self):
        """Records read so far: total, kept (past the filters), and the kept
        ones skipped for no SEQ or for a CIGAR whose query length differs from
        l_seq."""
        v = [ctypes.c_int64() for _ in range(4)]
        check(self._lib.mc_bases_src_counts(self._h, *[ctypes.byref(x) for x in v]), self._lib)
        return dict(zip(("records", "kept", "no_seq", "bad_cigar"), (x.value for x in v)))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mc_bases_src_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class GpuBaseSource:
    """The same records decoded on the GPU (mc_bam_gpu_open_bases): the whole
    file's read table, in mc_bases_add_batch's layout, resident in device
    memory until close.  BaseCounter.add_device feeds it; one open source
    serves any number of begins.  window_bytes: inflated bytes per decode
    window (0: the decoder's default)."""

    def __init__(self, path, device=0, n_threads=0, flag_filter=FLAG_FILTER, min_mapq=0, window_bytes=0, lib=None):
        from .bam import _header_of
        self._lib = lib or _lib.load()
        self._h = ctypes.c_void_p()
        self.device = int(device)
        check(self._lib.mc_bam_gpu_open_bases(str(path).encode(), self.device, int(n_threads), int(flag_filter),
                                              int(min_mapq), int(window_bytes), ctypes.byref(self._h)), self._lib)
        hdr = ctypes.c_void_p()
        check(self._lib.mc_bam_gpu_header(self._h, ctypes.byref(hdr)), self._lib)
        names, lengths, _ = _header_of(self._lib, hdr)
        self.references, self.lengths = list(names), list(lengths)
        # what add_device needs of the table: n, the sizes, the device pointers
        n, nw, sb, qb = (ctypes.c_int64() for _ in range(4))
        p = [ctypes.c_void_p() for _ in range(9)]
        r = ctypes.byref
        check(self._lib.mc_bam_gpu_bases_device(self._h, r(n), r(p[0]), r(p[1]), r(p[2]), r(p[3]), r(nw), r(p[4]),
                                                r(p[5]), r(p[6]), r(sb), r(p[7]), r(p[8]), r(qb)), self._lib)
        self.n = n.value
        self.n_words, self.seq_bytes, self.qual_bytes = nw.value, sb.value, qb.value
        self._dptr = [x.value or 0 for x in p]   # tid, pos, cig_off, cigar, l_seq, seq_off, seq, qual_off, qual
        f = ctypes.c_void_p()
        if hasattr(self._lib, "mc_bam_gpu_bases_flags"):             # (an A/B build of an older revision has none)
            check(self._lib.mc_bam_gpu_bases_flags(self._h, r(f)), self._lib)
        self._dflag = f.value or 0               # the flag column, uint16 per read
        f = ctypes.c_void_p()
        if hasattr(self._lib, "mc_bam_gpu_bases_mapq"):              # (the same)
            check(self._lib.mc_bam_gpu_bases_mapq(self._h, r(f)), self._lib)
        self._dmapq = f.value or 0               # the mapq column, uint8 per read
        self._lib.mc_bam_gpu_trim(self._h, None)  # the decode's staging is not needed again

    def __len__(self):
        return self.n

    def counts(self):
        """The whole file's record counts (BaseSource.counts at its end)."""
        v = [ctypes.c_int64() for _ in range(4)]
        check(self._lib.mc_bam_gpu_bases_counts(self._h, *[ctypes.byref(x) for x in v]), self._lib)
        return dict(zip(("records", "kept", "no_seq", "bad_cigar"), (x.value for x in v)))

    def timings(self):
        t = _lib.GpuDecodeTimings()
        check(self._lib.mc_bam_gpu_stats(self._h, ctypes.byref(t)), self._lib)
        return {k: getattr(t, k) for k, _ in t._fields_}

    def copy(self):
        """The read table on the host: a dict with BaseSource.next's keys."""
        n = self.n
        out = {"tid": np.zeros(n, np.int32), "pos": np.zeros(n, np.int32), "cig_off": np.zeros(n + 1, np.int64),
               "cigar": np.zeros(self.n_words, np.uint32), "l_seq": np.zeros(n, np.int32),
               "seq_off": np.zeros(n + 1, np.int64), "seq": np.zeros(self.seq_bytes, np.uint8),
               "qual_off": np.zeros(n + 1, np.int64), "qual": np.zeros(self.qual_bytes, np.uint8)}
        check(self._lib.mc_bam_gpu_bases_copy(self._h, *[ctypes.c_void_p(out[k].ctypes.data) if out[k].size else None
                                                         for k in ("tid", "pos", "cig_off", "cigar", "l_seq",
                                                                   "seq_off", "seq", "qual_off", "qual")]),
              self._lib)
        return out

    def copy_flags(self):
        """uint16 [n]: the reads' BAM flag words on the host."""
        out = np.zeros(self.n, np.uint16)
        check(self._lib.mc_bam_gpu_bases_copy_flags(self._h, ptr(out)), self._lib)
        return out

    def copy_mapq(self):
        """uint8 [n]: the reads' MAPQ bytes on the host."""
        out = np.zeros(self.n, np.uint8)
        check(self._lib.mc_bam_gpu_bases_copy_mapq(self._h, ptr(out)), self._lib)
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mc_bam_gpu_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class BaseCounter:
    """One mc_bases (device buffers that only grow, reused between begins)."""

    def __init__(self, n_ref, device=0, lib=None):
        self._lib = lib or _lib.load()
        self._h = ctypes.c_void_p()
        self.n_ref = int(n_ref)
        self.device = int(device)
        self._S = 0
        self.strand = False
        self._quality = False
        check(self._lib.mc_bases_create(self.device, self.n_ref, ctypes.byref(self._h)), self._lib)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mc_bases_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def begin(self, tids, starts, ends, min_baseq=0, insertions=False, strand=False, quality=False):
        """Allocates and zeroes the planes of the segments [start, end) of
        contig tid; returns N, the positions in all.  insertions: also collect
        the reads' insertion alleles (insertions(), consensus(insertions=True)).
        strand: also keep the reverse-strand reads' counts (counts_reverse(),
        sites(min_alt_strand=...)); the reads then come with their flags.
        quality: also keep the sums of the counted bases' quality bytes and of
        their reads' MAPQ (quality(), sites(min_alt_baseq=..., min_alt_mapq=...));
        the reads then come with their mapq column.  Not together with strand."""
        tids = np.ascontiguousarray(tids, dtype=np.int32)
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        ends = np.ascontiguousarray(ends, dtype=np.int64)
        if not len(tids) == len(starts) == len(ends):
            raise ValueError("tids / starts / ends lengths differ")
        check(self._lib.mc_bases_track_insertions(self._h, int(bool(insertions))), self._lib)
        if strand or hasattr(self._lib, "mc_bases_track_strand"):    # (an A/B build of an older revision has none)
            check(self._lib.mc_bases_track_strand(self._h, int(bool(strand))), self._lib)
        if quality or hasattr(self._lib, "mc_bases_track_quality"):  # (the same)
            check(self._lib.mc_bases_track_quality(self._h, int(bool(quality))), self._lib)
        self.strand = self._quality = False
        check(self._lib.mc_bases_begin(self._h, len(tids), ptr(tids), ptr(starts), ptr(ends), int(min_baseq)),
              self._lib)
        self.strand = bool(strand)
        self._quality = bool(quality)
        self._S = len(tids)
        return int(self.seg_off[-1])

    def add_reads(self, tid, pos, cig_off, cigar, l_seq, seq_off, seq, qual_off, qual, flag=None, mapq=None):
        """One batch of reads sorted by (tid, pos) (mc_bases_add_batch); flag:
        the reads' BAM flag words, required on a counter that tracks strand
        (mc_bases_add_batch_flags); mapq: their MAPQ bytes, required on one
        that tracks quality (mc_bases_add_batch_mapq)."""
        if self.strand and flag is None:
            raise ValueError("the counter tracks strand: add_reads needs the reads' flags")
        if self._quality and mapq is None:
            raise ValueError("the counter tracks quality: add_reads needs the reads' mapq")
        tid = np.ascontiguousarray(tid, dtype=np.int32)
        n = len(tid)
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        l_seq = np.ascontiguousarray(l_seq, dtype=np.int32)
        cig_off, seq_off, qual_off = (np.ascontiguousarray(a, dtype=np.int64) for a in (cig_off, seq_off, qual_off))
        cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        if len(pos) != n or len(l_seq) != n or any(len(a) != n + 1 for a in (cig_off, seq_off, qual_off)):
            raise ValueError("read arrays of inconsistent length")
        if n and (cig_off[n] > len(cigar) or seq_off[n] > len(seq) or qual_off[n] > len(qual)):
            raise ValueError("the last offset exceeds its arena")
        if mapq is not None and (self._quality or flag is None):
            mapq = np.ascontiguousarray(mapq, dtype=np.uint8)
            if len(mapq) != n:
                raise ValueError("read arrays of inconsistent length")
            check(self._lib.mc_bases_add_batch_mapq(self._h, n, ptr(tid), ptr(pos), ptr(cig_off), ptr(cigar),
                                                    ptr(l_seq), ptr(seq_off), ptr(seq), ptr(qual_off), ptr(qual),
                                                    ptr(mapq)), self._lib)
            return
        if flag is not None:
            flag = np.ascontiguousarray(flag, dtype=np.uint16)
            if len(flag) != n:
                raise ValueError("read arrays of inconsistent length")
            check(self._lib.mc_bases_add_batch_flags(self._h, n, ptr(tid), ptr(pos), ptr(cig_off), ptr(cigar),
                                                     ptr(l_seq), ptr(seq_off), ptr(seq), ptr(qual_off), ptr(qual),
                                                     ptr(flag)), self._lib)
            return
        check(self._lib.mc_bases_add_batch(self._h, n, ptr(tid), ptr(pos), ptr(cig_off), ptr(cigar), ptr(l_seq),
                                           ptr(seq_off), ptr(seq), ptr(qual_off), ptr(qual)), self._lib)

    def add_device(self, src, max_reads=1 << 20):
        """Every read of an open GpuBaseSource, straight from device memory
        (mc_bases_add_batch_device), in sub-ranges of max_reads reads of the
        resident table: add_bam's batch size, so one long read widens the
        tile search window of its own batch only."""
        if src.device != self.device:
            raise ValueError("the source is on device %d, the counter on device %d" % (src.device, self.device))
        if max_reads < 1:
            raise ValueError("max_reads must be positive")
        tid, pos, cig_off, cigar, l_seq, seq_off, seq, qual_off, qual = src._dptr

        def at(base, a, size):
            return ctypes.c_void_p(base + a * size) if base else None

        for a in range(0, src.n, int(max_reads)):
            n = min(int(max_reads), src.n - a)
            if self._quality:
                check(self._lib.mc_bases_add_batch_device_mapq(
                    self._h, n, at(tid, a, 4), at(pos, a, 4), at(cig_off, a, 8), at(cigar, 0, 4), src.n_words,
                    at(l_seq, a, 4), at(seq_off, a, 8), at(seq, 0, 1), src.seq_bytes, at(qual_off, a, 8),
                    at(qual, 0, 1), src.qual_bytes, at(src._dmapq, a, 1)), self._lib)
                continue
            if self.strand:
                check(self._lib.mc_bases_add_batch_device_flags(
                    self._h, n, at(tid, a, 4), at(pos, a, 4), at(cig_off, a, 8), at(cigar, 0, 4), src.n_words,
                    at(l_seq, a, 4), at(seq_off, a, 8), at(seq, 0, 1), src.seq_bytes, at(qual_off, a, 8),
                    at(qual, 0, 1), src.qual_bytes, at(src._dflag, a, 2)), self._lib)
                continue
            check(self._lib.mc_bases_add_batch_device(
                self._h, n, at(tid, a, 4), at(pos, a, 4), at(cig_off, a, 8), at(cigar, 0, 4), src.n_words,
                at(l_seq, a, 4), at(seq_off, a, 8), at(seq, 0, 1), src.seq_bytes, at(qual_off, a, 8),
                at(qual, 0, 1), src.qual_bytes), self._lib)
        if src.n == 0 and self._quality:
            check(self._lib.mc_bases_add_batch_device_mapq(self._h, 0, None, None, None, None, 0, None, None, None,
                                                           0, None, None, 0, None), self._lib)
        elif src.n == 0:     # (the state check of an empty batch, as add_reads makes it)
            check(self._lib.mc_bases_add_batch_device(self._h, 0, None, None, None, None, 0, None, None, None, 0,
                                                      None, None, 0), self._lib)

    def add_bam(self, path, flag_filter=FLAG_FILTER, min_mapq=0, max_reads=1 << 20, max_bases=1 << 27,
                n_threads=0, decode="host"):
        """Every kept record of a coordinate-sorted BAM, batch by batch;
        returns the source's record counts.  decode: "host" (BaseSource) or
        "gpu" (GpuBaseSource and add_device: the records never leave the
        device; max_bases does not apply)."""
        if decode not in ("host", "gpu"):
            raise ValueError("decode must be 'host' or 'gpu', not %r" % (decode,))
        if decode == "gpu":
            with GpuBaseSource(path, self.device, n_threads, flag_filter, min_mapq, lib=self._lib) as src:
                self.add_device(src, max_reads)
                return src.counts()
        with BaseSource(path, n_threads, flag_filter, min_mapq, self._lib) as src:
            while True:
                b = src.next(max_reads, max_bases)
                if b is None:
                    break
                self.add_reads(b["tid"], b["pos"], b["cig_off"], b["cigar"], b["l_seq"], b["seq_off"], b["seq"],
                               b["qual_off"], b["qual"], flag=src.flags() if self.strand else None,
                               mapq=src.mapq() if self._quality else None)
            return src.counts()

    @property
    def seg_off(self):
        """int64 [S + 1]: segment s owns plane indices seg_off[s] .. seg_off[s + 1]."""
        out = np.zeros(self._S + 1, np.int64)
        check(self._lib.mc_bases_seg_off(self._h, ptr(out)), self._lib)
        return out

    def counts(self, first=0, count=None):
        """uint32 [6, count]: the planes A, C, G, T, N, DEL over plane indices
        first .. first + count (default: all N)."""
        if count is None:
            count = int(self.seg_off[-1]) - int(first)
        out = np.zeros((6, max(int(count), 0)), np.uint32)
        check(self._lib.mc_bases_get(self._h, int(first), int(count), ptr(out)), self._lib)
        return out

    def counts_reverse(self, first=0, count=None):
        """uint32 [6, count]: the reverse-strand reads' share of counts() over
        the same plane indices; needs begin(..., strand=True)."""
        if count is None:
            count = int(self.seg_off[-1]) - int(first)
        out = np.zeros((6, max(int(count), 0)), np.uint32)
        check(self._lib.mc_bases_get_reverse(self._h, int(first), int(count), ptr(out)), self._lib)
        return out

    def quality(self, first=0, count=None):
        """(bq, mq), uint32 [6, count] each over the plane indices of
        counts(): the sums of the counted bases' quality bytes and of their
        reads' MAPQ bytes, per channel (bq[DEL] is 0); needs
        begin(..., quality=True).  A mean is the caller's division by
        counts()."""
        if count is None:
            count = int(self.seg_off[-1]) - int(first)
        bq = np.zeros((6, max(int(count), 0)), np.uint32)
        mq = np.zeros((6, max(int(count), 0)), np.uint32)
        check(self._lib.mc_bases_get_quality(self._h, int(first), int(count), ptr(bq), ptr(mq)), self._lib)
        return bq, mq

    def _ref_plane(self, ref):
        """ref (None, or uint8 [N] codes) as the library takes it: contiguous,
        one entry per position."""
        if ref is None:
            return None
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        if len(ref) != int(self.seg_off[-1]):
            raise ValueError("the reference plane must have one entry per position")
        return ref

    def _window_rows(self, first_fn, get_fn, n, cols):
        """(win_first, rows [n, cols]) of a window-row result through its
        mc_bases_*_first and mc_bases_*_get."""
        first = np.zeros(self._S + 1, np.int64)
        check(first_fn(self._h, ptr(first)), self._lib)
        rows = np.zeros((n, cols), np.int64)
        check(get_fn(self._h, 0, n, ptr(rows)), self._lib)
        return first, rows

    def sites(self, min_depth=1, min_count=1, min_ppm=0, ref=None, min_alt_strand=0, min_alt_baseq=0,
              min_alt_mapq=0):
        """The sites among the positions (see the header); ref: optional uint8
        [N], indexed like a plane, 0..3 = A/C/G/T, anything else unknown.
        min_alt_strand (needs begin(..., strand=True)): a site needs one
        alternative allele that passes min_count and min_ppm and is seen this
        many times on each strand.  On a counter that tracks strand the
        result carries rev_counts.  min_alt_baseq, min_alt_mapq (0..255, need
        begin(..., quality=True)): that allele's quality sum reaches
        min_alt_baseq times its count (DEL exempt) and its MAPQ sum
        min_alt_mapq times its count.  On a counter that tracks quality the
        result carries bq_sums and mq_sums."""
        if min_alt_strand and not self.strand:
            raise ValueError("min_alt_strand needs a counter that tracks strand (begin(..., strand=True))")
        if (min_alt_baseq or min_alt_mapq) and not self._quality:
            raise ValueError("min_alt_baseq / min_alt_mapq need a counter that tracks quality "
                             "(begin(..., quality=True))")
        ref = self._ref_plane(ref)
        n = ctypes.c_int64()
        if self._quality:
            check(self._lib.mc_bases_sites_quality(self._h, int(min_depth), int(min_count), int(min_ppm),
                                                   int(min_alt_baseq), int(min_alt_mapq), ptr(ref),
                                                   ctypes.byref(n)), self._lib)
        elif self.strand:
            check(self._lib.mc_bases_sites_strand(self._h, int(min_depth), int(min_count), int(min_ppm),
                                                  int(min_alt_strand), ptr(ref), ctypes.byref(n)), self._lib)
        else:
            check(self._lib.mc_bases_sites(self._h, int(min_depth), int(min_count), int(min_ppm), ptr(ref),
                                           ctypes.byref(n)), self._lib)
        n = n.value
        first = np.zeros(self._S + 1, np.int64)
        check(self._lib.mc_bases_sites_first(self._h, ptr(first)), self._lib)
        pos = np.zeros(n, np.int64)
        cnt = np.zeros((n, 6), np.uint32)
        check(self._lib.mc_bases_sites_get(self._h, 0, n, ptr(pos), ptr(cnt)), self._lib)
        rev = None
        if self.strand:
            rev = np.zeros((n, 6), np.uint32)
            check(self._lib.mc_bases_sites_get_reverse(self._h, 0, n, ptr(rev)), self._lib)
        bq = mq = None
        if self._quality:
            bq, mq = np.zeros((n, 6), np.uint32), np.zeros((n, 6), np.uint32)
            check(self._lib.mc_bases_sites_get_quality(self._h, 0, n, ptr(bq), ptr(mq)), self._lib)
        return Sites(first, pos, cnt, rev, bq, mq)

    def insertions(self, min_depth=1, min_count=1, min_ppm=0):
        """The grouped insertion alleles (see the header, "Insertion alleles")
        that pass the sites predicate with their own count; needs
        begin(..., insertions=True).  Returns an Insertions."""
        n = ctypes.c_int64()
        check(self._lib.mc_bases_insertions(self._h, int(min_depth), int(min_count), int(min_ppm), ctypes.byref(n)),
              self._lib)
        n = n.value
        first = np.zeros(self._S + 1, np.int64)
        check(self._lib.mc_bases_insertions_first(self._h, ptr(first)), self._lib)
        index, length, code = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.uint64)
        other, count = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        check(self._lib.mc_bases_insertions_get(self._h, 0, n, ptr(index), ptr(length), ptr(code), ptr(other),
                                                ptr(count)), self._lib)
        return Insertions(first, index, length, code, other, count)

    def set_insertions(self, index, length, code, other, count):
        """Test hook (mc_bases_ins_set): installs a grouped allele table, rows
        sorted by (index, other, length, code) and unique, in place of the
        reads' events."""
        index = np.ascontiguousarray(index, dtype=np.int64)
        length = np.ascontiguousarray(length, dtype=np.int32)
        code = np.ascontiguousarray(code, dtype=np.uint64)
        other = np.ascontiguousarray(other, dtype=np.uint8)
        count = np.ascontiguousarray(count, dtype=np.uint32)
        if not len(index) == len(length) == len(code) == len(other) == len(count):
            raise ValueError("row arrays of inconsistent length")
        check(self._lib.mc_bases_ins_set(self._h, len(index), ptr(index), ptr(length), ptr(code), ptr(other),
                                         ptr(count)), self._lib)

    def insertions_timing(self):
        a, b, c, n = ctypes.c_float(), ctypes.c_float(), ctypes.c_float(), ctypes.c_int64()
        check(self._lib.mc_bases_insertions_timing(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                                                   ctypes.byref(n)), self._lib)
        return {"extract_ms": a.value, "group_ms": b.value, "consensus_ms": c.value, "events": n.value}

    def set_counts(self, first, planes, rev=None, bq=None, mq=None):
        """Test hook (mc_bases_set): overwrites plane indices first .. first +
        count with planes, uint32 [6, count]; sites and consensus results are
        gone afterwards.  rev (mc_bases_set_strand, needs strand=True): the
        reverse planes of the same range, rev <= planes everywhere.  bq, mq
        (mc_bases_set_quality, needs quality=True; both or neither): the sum
        planes of the same range, at most 255 x planes, bq[DEL] zero."""
        planes = np.ascontiguousarray(planes, dtype=np.uint32)
        if planes.ndim != 2 or planes.shape[0] != 6:
            raise ValueError("planes must be [6, count]")
        if (bq is None) != (mq is None):
            raise ValueError("bq and mq come together")
        if bq is not None:
            bq = np.ascontiguousarray(bq, dtype=np.uint32)
            mq = np.ascontiguousarray(mq, dtype=np.uint32)
            if bq.shape != planes.shape or mq.shape != planes.shape:
                raise ValueError("bq and mq must have the shape of planes")
            check(self._lib.mc_bases_set_quality(self._h, int(first), planes.shape[1], ptr(planes), ptr(bq),
                                                 ptr(mq)), self._lib)
            return
        if rev is not None:
            rev = np.ascontiguousarray(rev, dtype=np.uint32)
            if rev.shape != planes.shape:
                raise ValueError("rev must have the shape of planes")
            check(self._lib.mc_bases_set_strand(self._h, int(first), planes.shape[1], ptr(planes), ptr(rev)),
                  self._lib)
            return
        check(self._lib.mc_bases_set(self._h, int(first), planes.shape[1], ptr(planes)), self._lib)

    def consensus(self, min_depth=1, min_count=1, call_ppm=0, iupac=False, fill_ref=False, ref=None,
                  insertions=False):
        """One letter per position, called on the device (see the header,
        "Consensus"); ref: optional uint8 [N] codes as sites takes them.
        insertions: the called insertion alleles follow their anchor's letter
        in the compact output (needs begin(..., insertions=True)).
        Returns a Consensus; its letters stay on the device until fetched."""
        ref = self._ref_plane(ref)
        flags = (CONS_IUPAC if iupac else 0) | (CONS_FILL_REF if fill_ref else 0) | (CONS_INS if insertions else 0)
        n = ctypes.c_int64()
        # (an empty plane still counts as given: FILL_REF with N == 0 is valid)
        p = None if ref is None else ctypes.c_void_p(ref.ctypes.data)
        check(self._lib.mc_bases_consensus(self._h, int(min_depth), int(min_count), int(call_ppm), flags, p,
                                           ctypes.byref(n)), self._lib)
        first = np.zeros(self._S + 1, np.int64)
        check(self._lib.mc_bases_consensus_first(self._h, ptr(first)), self._lib)
        summary = np.zeros((self._S, CONS_COLS), np.int64)
        check(self._lib.mc_bases_consensus_summary(self._h, ptr(summary)), self._lib)
        inserted = None
        if insertions:
            inserted = np.zeros((self._S, 2), np.int64)
            check(self._lib.mc_bases_consensus_ins(self._h, ptr(inserted)), self._lib)
        return Consensus(self, self.seg_off, first, summary, n.value, inserted)

    def consensus_letters(self, compact, first, count):
        """uint8 [count] of the aligned (compact false) or compact letters,
        copied GET_CHUNK at a time."""
        out = np.zeros(max(int(count), 0), np.uint8)
        if count <= 0:
            check(self._lib.mc_bases_consensus_get(self._h, int(bool(compact)), int(first), int(count), None),
                  self._lib)
        for a in range(0, int(count), GET_CHUNK):
            n = min(GET_CHUNK, int(count) - a)
            check(self._lib.mc_bases_consensus_get(self._h, int(bool(compact)), int(first) + a, n,
                                                   ctypes.c_void_p(out.ctypes.data + a)), self._lib)
        return out

    def consensus_timing(self):
        a, b, c = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        check(self._lib.mc_bases_consensus_timing(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
              self._lib)
        return {"call_ms": a.value, "scan_ms": b.value, "emit_ms": c.value}

    def diversity(self, window=0, min_depth=2, min_count=1, min_ppm=0, ref=None):
        """Per window of `window` positions of each segment (0: per segment)
        the eight sums of the header's "Diversity", reduced on the device;
        ref: optional uint8 [N] codes as sites takes them.  Returns a
        Diversity."""
        ref = self._ref_plane(ref)
        n = ctypes.c_int64()
        check(self._lib.mc_bases_diversity(self._h, int(window), int(min_depth), int(min_count), int(min_ppm),
                                           ptr(ref), ctypes.byref(n)), self._lib)
        return Diversity(*self._window_rows(self._lib.mc_bases_diversity_first, self._lib.mc_bases_diversity_get,
                                            n.value, DIV_COLS), window)

    def diversity_timing(self):
        """HIP-event times of the last diversity call: the tile kernel, and
        the launch in front of it that zeroes the rows tiles share."""
        a, b = ctypes.c_float(), ctypes.c_float()
        check(self._lib.mc_bases_diversity_timing(self._h, ctypes.byref(a), ctypes.byref(b)), self._lib)
        return {"tile_ms": a.value, "combine_ms": b.value}

    def compare(self, other, window=0, min_depth=2, min_count=1, min_ppm=0):
        """This counter's sample against `other`'s, both begun on the same
        segments of one device: per window of `window` positions of each
        segment (0: per segment) the eight sums of the header's "Comparison",
        reduced on the device from both counters' planes.  The result belongs
        to this counter; `other` is only read.  Returns a Comparison."""
        if not isinstance(other, BaseCounter):
            raise TypeError("compare takes another BaseCounter")
        n = ctypes.c_int64()
        check(self._lib.mc_bases_compare(self._h, other._h, int(window), int(min_depth), int(min_count),
                                         int(min_ppm), ctypes.byref(n)), self._lib)
        return Comparison(*self._window_rows(self._lib.mc_bases_compare_first, self._lib.mc_bases_compare_get,
                                             n.value, CMP_COLS), window)

    def compare_timing(self):
        """HIP-event times of the last compare call: the tile kernel, and the
        launch in front of it that zeroes the rows tiles share."""
        a, b = ctypes.c_float(), ctypes.c_float()
        check(self._lib.mc_bases_compare_timing(self._h, ctypes.byref(a), ctypes.byref(b)), self._lib)
        return {"tile_ms": a.value, "zero_ms": b.value}

    def timing(self):
        a, b, c = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        t, r = ctypes.c_int64(), ctypes.c_int64()
        check(self._lib.mc_bases_timing(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(t),
                                        ctypes.byref(r)), self._lib)
        return {"prepass_ms": a.value, "pileup_ms": b.value, "sites_ms": c.value, "tiles": t.value,
                "reads": r.value}


def count_coverage(path, contig, start=None, stop=None, quality_threshold=15, min_mapq=0, device=0, decode="host"):
    """pysam's AlignmentFile.count_coverage(contig, start, stop,
    quality_threshold) with read_callback='all': four uint32 arrays A, C, G, T
    of stop - start counts (default: the whole contig).  decode: as add_bam."""
    if decode not in ("host", "gpu"):
        raise ValueError("decode must be 'host' or 'gpu', not %r" % (decode,))
    lib = _lib.load()
    names, tid, start, stop, _ = _one_segment(path, contig, start, stop, min_mapq, lib)
    with BaseCounter(len(names), device, lib) as bc:
        bc.begin([tid], [start], [stop], min_baseq=quality_threshold)
        bc.add_bam(path, min_mapq=min_mapq, decode=decode)
        planes = bc.counts()
    return planes[A].copy(), planes[C].copy(), planes[G].copy(), planes[T].copy()


def _one_segment(path, contig, start, stop, min_mapq, lib, ref=None):
    """What the one-call functions make of their arguments: (names, tid,
    start, stop, codes) of [start, stop) of `contig` in path's header (default:
    all of it); codes: the reference plane of ref, ASCII letters (str, bytes or
    uint8) of the same range, or None."""
    with BaseSource(path, 0, FLAG_FILTER, min_mapq, lib) as src:
        names = contig_names(src.references)
        if contig not in names:
            raise KeyError("contig '%s' is not in the header of %s" % (contig, path))
        tid = names.index(contig)
        length = src.lengths[tid]
    start = 0 if start is None else int(start)
    stop = length if stop is None else int(stop)
    if start < 0 or stop < start:
        raise ValueError("bad range [%d, %d)" % (start, stop))
    codes = None
    if ref is not None:
        if isinstance(ref, str):
            ref = ref.encode("ascii")
        codes = ref_codes(np.frombuffer(ref, np.uint8) if isinstance(ref, (bytes, bytearray)) else ref)
        if len(codes) != stop - start:
            raise ValueError("ref must have stop - start letters")
    return names, tid, start, stop, codes


# ------------------------------------------------------------------ output

HEADER = "contig\tpos\tref\tdepth\tA\tC\tG\tT\tN\tDEL\n"
HEADER_STRAND = (HEADER[:-1] + "".join("\t%s_fwd" % c for c in CHANNELS) +
                 "".join("\t%s_rev" % c for c in CHANNELS) + "\n")
HEADER_QUALITY = (HEADER[:-1] + "".join("\t%s_bq" % c for c in CHANNELS[:5]) +
                  "".join("\t%s_mq" % c for c in CHANNELS) + "\n")
_REF_CODE = np.full(256, 4, np.uint8)
for _i, _ch in enumerate("ACGT"):
    _REF_CODE[ord(_ch)] = _REF_CODE[ord(_ch.lower())] = _i


def ref_codes(letters):
    """uint8 ASCII letters -> the reference plane's codes (0..3, 4 = other)."""
    return _REF_CODE[np.asarray(letters, np.uint8)]


def write_sites(fh, name, pos, counts, ref=None, rev=None, bq=None, mq=None):
    """Tab-separated `contig pos ref depth A C G T N DEL` lines of one contig:
    pos [n] 0-based positions (written 1-based, as mpileup and VCF), counts
    [n, 6], ref [n] uint8 ASCII letters or None ('.').  depth = A + C + G + T
    + DEL.  rev [n, 6] (the reverse-strand share of counts): twelve more
    columns, the six forward counts (counts - rev) and the six reverse ones
    (HEADER_STRAND).  bq, mq [n, 6] (the quality and MAPQ sums behind counts,
    both or neither): eleven more columns of exact integer sums, A_bq .. N_bq
    and A_mq .. DEL_mq (HEADER_QUALITY); a mean is the reader's division by the
    count.  Returns the lines written."""
    pos = np.asarray(pos, np.int64)
    n = len(pos)
    if n == 0:
        return 0
    counts = np.asarray(counts).reshape(n, 6).astype(np.int64)
    depth = counts[:, [A, C, G, T, DEL]].sum(axis=1)
    if ref is None:
        letters = np.full(n, ".", dtype="U1")
    else:
        letters = np.char.upper(np.asarray(ref, np.uint8).view("S1").astype("U1"))
    line = np.char.add(str(name) + "\t", (pos + 1).astype(str))
    line = np.char.add(np.char.add(line, "\t"), letters)
    cols = [depth] + [counts[:, c] for c in range(6)]
    if rev is not None:
        rev = np.asarray(rev).reshape(n, 6).astype(np.int64)
        cols += [counts[:, c] - rev[:, c] for c in range(6)] + [rev[:, c] for c in range(6)]
    if (bq is None) != (mq is None):
        raise ValueError("bq and mq come together")
    if bq is not None:
        bq = np.asarray(bq).reshape(n, 6).astype(np.int64)
        mq = np.asarray(mq).reshape(n, 6).astype(np.int64)
        cols += [bq[:, c] for c in range(5)] + [mq[:, c] for c in range(6)]
    for col in cols:
        line = np.char.add(np.char.add(line, "\t"), col.astype(str))
    fh.write("\n".join(line.tolist()))
    fh.write("\n")
    return n


INSERTIONS_HEADER = "contig\tpos\tdepth\tcount\tlen\tseq\n"


def write_insertions(fh, name, pos, depth, count, length, seqs):
    """Tab-separated `contig pos depth count len seq` lines of one contig:
    pos [n] 0-based anchors (written 1-based, as write_sites), depth the
    anchor's A + C + G + T + DEL, seqs the inserted bases ('*' with len 0 for
    the OTHER row).  Returns the lines written."""
    n = len(pos)
    for k in range(n):
        fh.write("%s\t%d\t%d\t%d\t%d\t%s\n" % (name, int(pos[k]) + 1, int(depth[k]), int(count[k]),
                                               int(length[k]), seqs[k]))
    return n


# --------------------------------------------------------------- consensus

SUMMARY_HEADER = "contig\tstart\tend\t" + "\t".join(SUMMARY_COLUMNS) + "\n"


def write_fasta(fh, name, letters, width=60):
    """One FASTA record: `>name`, then the uint8 ASCII letters in lines of
    `width` (0: one line), wrapped in numpy.  An empty sequence writes the
    header alone."""
    letters = np.asarray(letters, np.uint8).reshape(-1)
    n = len(letters)
    fh.write(">%s\n" % name)
    if n == 0:
        return
    if width <= 0 or n <= width:
        fh.write(letters.tobytes().decode("ascii"))
        fh.write("\n")
        return
    full, rest = divmod(n, int(width))
    out = np.empty(n + full + (1 if rest else 0), np.uint8)
    body = out[:full * (width + 1)].reshape(full, width + 1)
    body[:, :width] = letters[:full * width].reshape(full, width)
    body[:, width] = 10
    if rest:
        out[full * (width + 1):-1] = letters[full * width:]
        out[-1] = 10
    fh.write(out.tobytes().decode("ascii"))


SUMMARY_HEADER_INS = SUMMARY_HEADER[:-1] + "\tinsertions\tinserted\n"


def write_consensus_summary(fh, names, starts, ends, summary, header=True, inserted=None):
    """Tab-separated `contig start end positions called ambiguous nocall low
    deleted differs length`, one line per segment (start, end 0-based,
    half-open); inserted (Consensus.inserted): two trailing columns
    `insertions inserted`.  Returns the lines written."""
    if header:
        fh.write(SUMMARY_HEADER if inserted is None else SUMMARY_HEADER_INS)
    summary = np.asarray(summary, np.int64).reshape(-1, CONS_COLS)
    if inserted is not None:
        summary = np.concatenate([summary, np.asarray(inserted, np.int64).reshape(-1, 2)], axis=1)
    for name, a, b, row in zip(names, starts, ends, summary.tolist()):
        fh.write("%s\t%d\t%d\t%s\n" % (name, int(a), int(b), "\t".join(str(v) for v in row)))
    return len(summary)


DIVERSITY_HEADER = ("#contig\tstart\tend\tpositions\tcovered\tbases\tsnv\tpi\tcompared\tcon_diff\tpop_diff\t"
                    "con_ani\tpop_ani\n")


def write_diversity(fh, names, starts, diversity, header=True):
    """Tab-separated `contig start end positions covered bases snv pi compared
    con_diff pop_diff con_ani pop_ani`, one line per window: names and starts
    per segment (start, end 0-based, half-open, in the contig's coordinates);
    the integers as they are, pi and the two identities '%.6f', or NA where
    their denominator is 0.  Returns the lines written."""
    d = diversity
    return _write_window_rows(fh, DIVERSITY_HEADER if header else None, names, starts, d,
                              [0, 1, 2, 3, d.pi(), 5, 6, 7, d.con_ani(), d.pop_ani()])


def _write_window_rows(fh, header, names, starts, d, columns):
    """The table of write_diversity and write_compare: `header` (or None),
    then per row of d `contig start end` and the columns, each an index into
    the row (an integer as it is) or a float64 array with one value per row
    ('%.6f', or NA for NaN).  Returns the lines written."""
    if header:
        fh.write(header)
    seg = d.segment()
    a = d.start() + np.asarray(starts, np.int64).reshape(-1)[seg] if len(d) else np.zeros(0, np.int64)
    b = a + d.positions
    line = "%s\t%d\t%d" + "".join("\t%d" if isinstance(c, int) else "\t%s" for c in columns) + "\n"
    cells = [d.rows[:, c].tolist() if isinstance(c, int) else ["NA" if np.isnan(v) else "%.6f" % v for v in c]
             for c in columns]
    for k, row in enumerate(zip(*cells)):
        fh.write(line % ((names[int(seg[k])], int(a[k]), int(b[k])) + row))
    return len(d)


def diversity(path, contig, start=None, stop=None, window=0, quality_threshold=0, min_mapq=0, min_depth=2,
              min_count=1, min_ppm=0, ref=None, device=0, decode="host"):
    """The diversity rows of [start, stop) of one contig (default: all of it)
    in one call: a Diversity of one segment, cut into windows of `window`
    positions (0: one row).  ref: optional ASCII letters (str, bytes or uint8)
    of the same range.  decode: as add_bam."""
    if decode not in ("host", "gpu"):
        raise ValueError("decode must be 'host' or 'gpu', not %r" % (decode,))
    if window != 0 and window < DIV_MIN_WINDOW:
        raise ValueError("window must be 0 or at least %d" % DIV_MIN_WINDOW)
    lib = _lib.load()
    names, tid, start, stop, codes = _one_segment(path, contig, start, stop, min_mapq, lib, ref)
    with BaseCounter(len(names), device, lib) as bc:
        bc.begin([tid], [start], [stop], min_baseq=quality_threshold)
        bc.add_bam(path, min_mapq=min_mapq, decode=decode)
        return bc.diversity(window, min_depth, min_count, min_ppm, codes)


COMPARE_HEADER = ("#contig\tstart\tend\tpositions\tcovered_a\tcovered_b\tcompared\tcon_diff\tpop_diff\tsnv\t"
                  "con_ani\tpop_ani\taf_dist\n")


def write_compare(fh, names, starts, comparison, header=True):
    """Tab-separated `contig start end positions covered_a covered_b compared
    con_diff pop_diff snv con_ani pop_ani af_dist`, one line per window: names
    and starts per segment (start, end 0-based, half-open, in the contig's
    coordinates); the integers as they are, the two identities and the mean
    allele-frequency distance '%.6f', or NA where nothing was compared.
    Returns the lines written."""
    d = comparison
    return _write_window_rows(fh, COMPARE_HEADER if header else None, names, starts, d,
                              [0, 1, 2, 3, 4, 5, 6, d.con_ani(), d.pop_ani(), d.distance()])


def same_references(path_a, refs_a, lens_a, path_b, refs_b, lens_b):
    """None where the two headers name the same references with the same
    lengths in the same order, else a sentence naming the first difference."""
    if len(refs_a) != len(refs_b):
        return "%s has %d references, %s has %d" % (path_a, len(refs_a), path_b, len(refs_b))
    for i, (ra, la, rb, lb) in enumerate(zip(refs_a, lens_a, refs_b, lens_b)):
        if ra != rb or la != lb:
            return "reference %d is '%s' (%d bp) in %s and '%s' (%d bp) in %s" % (i, ra, la, path_a, rb, lb, path_b)
    return None


def compare(path_a, path_b, contig, start=None, stop=None, window=0, quality_threshold=0, min_mapq=0, min_depth=2,
            min_count=1, min_ppm=0, device=0, decode="host"):
    """The comparison rows of two BAMs over [start, stop) of one contig
    (default: all of it) in one call: a Comparison of one segment, cut into
    windows of `window` positions (0: one row).  Both files must have the same
    references.  decode: as add_bam."""
    if decode not in ("host", "gpu"):
        raise ValueError("decode must be 'host' or 'gpu', not %r" % (decode,))
    if window != 0 and window < DIV_MIN_WINDOW:
        raise ValueError("window must be 0 or at least %d" % DIV_MIN_WINDOW)
    lib = _lib.load()
    with BaseSource(path_a, 0, FLAG_FILTER, min_mapq, lib) as src, \
            BaseSource(path_b, 0, FLAG_FILTER, min_mapq, lib) as src_b:
        diff = same_references(path_a, src.references, src.lengths, path_b, src_b.references, src_b.lengths)
        if diff:
            raise ValueError(diff)
    names, tid, start, stop, _ = _one_segment(path_a, contig, start, stop, min_mapq, lib)
    with BaseCounter(len(names), device, lib) as bc, BaseCounter(len(names), device, lib) as other:
        for h, path in ((bc, path_a), (other, path_b)):
            h.begin([tid], [start], [stop], min_baseq=quality_threshold)
            h.add_bam(path, min_mapq=min_mapq, decode=decode)
        return bc.compare(other, window, min_depth, min_count, min_ppm)


def consensus(path, contig, start=None, stop=None, quality_threshold=0, min_mapq=0, min_depth=1, min_count=1,
              call_ppm=0, iupac=False, fill_ref=False, ref=None, aligned=False, device=0, decode="host",
              insertions=False):
    """The consensus of [start, stop) of one contig (default: all of it) in
    one call: (letters uint8, summary int64 [8]).  aligned: keep '-' for the
    deleted positions, one letter per reference position.  ref: optional
    ASCII letters (str, bytes or uint8) of the same range.  decode: as
    add_bam.  insertions: the compact letters include the called insertion
    alleles (not with aligned: that output has one letter per position)."""
    if decode not in ("host", "gpu"):
        raise ValueError("decode must be 'host' or 'gpu', not %r" % (decode,))
    if insertions and aligned:
        raise ValueError("insertions has no place in the aligned output")
    lib = _lib.load()
    names, tid, start, stop, codes = _one_segment(path, contig, start, stop, min_mapq, lib, ref)
    with BaseCounter(len(names), device, lib) as bc:
        bc.begin([tid], [start], [stop], min_baseq=quality_threshold, insertions=insertions)
        bc.add_bam(path, min_mapq=min_mapq, decode=decode)
        c = bc.consensus(min_depth, min_count, call_ppm, iupac, fill_ref, codes, insertions=insertions)
        return (c.aligned(0) if aligned else c.compact(0)), c.summary[0].copy()
