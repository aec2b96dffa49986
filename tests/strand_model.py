"""Model of the strand-resolved base counts (include/metacov_amd.h, "Strand"),
pure Python / numpy over tests/bases_model.py, restated from the contract and
not from the library's code:

strand     a read is on the reverse strand iff flag & 0x10; no other bit matters
counts     every count a read makes (A C G T N DEL) belongs to its strand; the
           six planes are the totals, rev[6][N] the reverse reads' share,
           forward = total - rev
sites      depth and the base allele as bases_model.sites_model; a site iff
           depth >= min_depth and some allele i != base (of A C G T DEL) has
           a[i] >= min_count, a[i] * 10^6 >= min_ppm * depth,
           fwd[i] >= min_alt_strand and rev[i] >= min_alt_strand
"""
import numpy as np

from tests import bases_model as bm
from tests.bases_model import A, C, G, T, DEL

REVERSE = 0x10
STRAND_COLUMNS = ["%s_fwd" % c for c in "A C G T N DEL".split()] + ["%s_rev" % c for c in "A C G T N DEL".split()]


def is_reverse(flag):
    return (np.asarray(flag, np.int64) & REVERSE) != 0


def reads_of(batches, flags, reverse):
    """The reads of one strand, each as a one-read batch."""
    if isinstance(batches, dict):
        batches, flags = [batches], [flags]
    out = []
    for b, f in zip(batches, flags):
        assert len(f) == bm.n_reads(b)
        out += [bm.slice_batch(b, int(i), int(i) + 1) for i in np.flatnonzero(is_reverse(f) == reverse)]
    return out


def counts_model(batches, flags, tids, starts, ends, min_baseq=0, loop=False):
    """(seg_off, total uint32 [6, N], rev uint32 [6, N]); loop: the literal
    per-base loop of bases_model.counts_loop in place of its event model."""
    count = bm.counts_loop if loop else bm.counts_model
    seg_off, fwd = count(reads_of(batches, flags, False), tids, starts, ends, min_baseq)
    _, rev = count(reads_of(batches, flags, True), tids, starts, ends, min_baseq)
    return seg_off, (fwd + rev).astype(np.uint32), rev.astype(np.uint32)


def sites_model(total, rev, seg_off, starts, min_depth=1, min_count=1, min_ppm=0, min_alt_strand=0, ref=None):
    """(site_first [S + 1], site_pos int64, site_counts uint32 [n, 6],
    site_rev uint32 [n, 6]), position by position."""
    total, rev = np.asarray(total, np.int64), np.asarray(rev, np.int64)
    alleles = [A, C, G, T, DEL]
    hits = []
    for p in range(total.shape[1]):
        a = [int(total[c, p]) for c in alleles]
        r = [int(rev[c, p]) for c in alleles]
        depth = sum(a)
        base = a.index(max(a))                                  # the first maximum: the lowest channel
        if ref is not None and int(ref[p]) < 4:
            base = int(ref[p])
        ok = any(i != base and a[i] >= min_count and a[i] * 1000000 >= min_ppm * depth and
                 a[i] - r[i] >= min_alt_strand and r[i] >= min_alt_strand for i in range(5))
        if depth >= min_depth and ok:
            hits.append(p)
    idx = np.array(hits, np.int64)
    first = np.searchsorted(idx, np.asarray(seg_off, np.int64)).astype(np.int64)
    pos = np.zeros(len(idx), np.int64)
    for s in range(len(starts)):
        x, y = int(first[s]), int(first[s + 1])
        pos[x:y] = idx[x:y] - int(seg_off[s]) + int(starts[s])
    return (first, pos, total[:, idx].T.astype(np.uint32).reshape(-1, 6),
            rev[:, idx].T.astype(np.uint32).reshape(-1, 6))


def kept_flags(path, flag_filter=bm.FLAG_FILTER, min_mapq=0):
    """uint16 flags of the records bases_model.kept_reads hands out, in its order."""
    _, _, recs = bm.read_bam(path)
    out = []
    for r in recs:
        if r["tid"] < 0 or (r["flag"] & flag_filter) or r["mapq"] < min_mapq:
            continue
        if r["l_seq"] == 0 or bm.query_length(r["cigar"]) != r["l_seq"]:
            continue
        out.append(r["flag"])
    return np.array(out, np.uint16)


def table(name_of, rows, fasta=None):
    """The `bases --strand` table: rows of (tid, 0-based pos, six totals, six
    reverse counts)."""
    plain = bm.table(name_of, [(t, p, c) for t, p, c, _ in rows], fasta).split("\n")[:-1]
    out = [plain[0] + "\t" + "\t".join(STRAND_COLUMNS)]
    for line, (_, _, c, r) in zip(plain[1:], rows):
        c, r = [int(x) for x in c], [int(x) for x in r]
        out.append(line + "\t" + "\t".join(str(x - y) for x, y in zip(c, r)) + "\t" + "\t".join(str(y) for y in r))
    return "\n".join(out) + "\n"
