"""Model of the per-position base counts (include/metacov_amd.h, "per-position
base counts"), pure Python / numpy, restated from the contract and not from
the library's code:

reads      a batch in mc_bases_add_batch's layout (a dict of arrays)
walk       from rpos = pos, qpos = 0: M/=/X count the base at (qpos, rpos)
           and advance both; D counts DEL at each rpos; N advances rpos; I/S
           advance qpos; H/P and unassigned ops do nothing
channels   A C G T N DEL = 0..5; nt16 1/2/4/8 -> A/C/G/T, everything else N
quality    min_baseq > 0: a base below it counts nothing, unless the read's
           first quality byte is 0xFF; DEL is never tested
segments   planes[6][N], plane index seg_off[s] + (p - start[s])
sites      depth = A+C+G+T+DEL; base = ref allele where ref < 4 else argmax
           (ties: lowest channel); alt = max of the other four; site iff
           depth >= min_depth, alt >= min_count, alt * 10^6 >= min_ppm * depth

It carries its own BAM reader (gzip + struct) with MAPQ, SEQ and QUAL.
"""
import gzip
import re
import struct

import numpy as np

A, C, G, T, N, DEL = range(6)
OPS = "MIDNSHP=X"
QUERY_OPS = {0, 1, 4, 7, 8}
REF_OPS = {0, 2, 3, 7, 8}
NT16 = "=ACMGRSVTWYHKDBN"
CHANNEL_OF_CODE = [N, A, C, N, G, N, N, N, T, N, N, N, N, N, N, N]
FLAG_FILTER = 0x704


# ------------------------------------------------------------------ batches

def cigar_words(cigar):
    """'3S5M2D' or [(op, len), ...] or packed words -> uint32 words."""
    if isinstance(cigar, str):
        return np.array([(int(n) << 4) | OPS.index(op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)],
                        np.uint32)
    cigar = list(cigar)
    if cigar and isinstance(cigar[0], tuple):
        return np.array([(int(n) << 4) | int(op) for op, n in cigar], np.uint32)
    return np.array(cigar, np.uint32)


def query_length(words):
    return int(sum(int(w) >> 4 for w in words if (int(w) & 15) in QUERY_OPS))


def ref_span(words):
    return int(sum(int(w) >> 4 for w in words if (int(w) & 15) in REF_OPS))


def pack_seq(codes):
    """nt16 codes (or a letter string) -> bytes, two per byte, high nibble first."""
    if isinstance(codes, str):
        codes = [NT16.index(ch) if ch in NT16 else 15 for ch in codes.upper()]
    codes = list(codes) + [0] * (len(codes) & 1)
    return bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2))


def make_batch(reads, seq_gap=0, qual_gap=0, l_seq=None):
    """reads: (tid, pos, cigar, bases, quals) tuples; bases a letter string or
    nt16 codes; quals a sequence, one int for all, or None (0xFF: absent).
    seq_gap / qual_gap: unused bytes in front of every read in its arena (odd
    values put reads at odd byte offsets).  l_seq: override (invalid batches)."""
    tid, pos, ls, cig, cig_off, seq, seq_off, qual, qual_off = [], [], [], [], [0], bytearray(), [], bytearray(), []
    for k, (t, p, c, bases, q) in enumerate(reads):
        w = cigar_words(c)
        n = len(bases)
        if q is None:
            q = [0xFF] * n
        elif np.isscalar(q):
            q = [int(q)] * n
        assert len(q) == n
        tid.append(t)
        pos.append(p)
        ls.append(n if l_seq is None else l_seq[k])
        cig.extend(int(x) for x in w)
        cig_off.append(len(cig))
        seq.extend(b"\xAA" * seq_gap)
        seq_off.append(len(seq))
        seq.extend(pack_seq(bases))
        qual.extend(b"\x00" * qual_gap)
        qual_off.append(len(qual))
        qual.extend(bytes(q))
    seq_off.append(len(seq))
    qual_off.append(len(qual))
    return {"tid": np.array(tid, np.int32), "pos": np.array(pos, np.int32), "l_seq": np.array(ls, np.int32),
            "cig_off": np.array(cig_off, np.int64), "cigar": np.array(cig, np.uint32),
            "seq_off": np.array(seq_off, np.int64), "seq": np.frombuffer(bytes(seq), np.uint8).copy(),
            "qual_off": np.array(qual_off, np.int64), "qual": np.frombuffer(bytes(qual), np.uint8).copy()}


def slice_batch(b, lo, hi):
    """Reads [lo, hi) of a batch as a batch of their own (arenas re-based)."""
    c0, c1 = int(b["cig_off"][lo]), int(b["cig_off"][hi])
    s0, s1 = int(b["seq_off"][lo]), int(b["seq_off"][hi])
    q0, q1 = int(b["qual_off"][lo]), int(b["qual_off"][hi])
    return {"tid": b["tid"][lo:hi].copy(), "pos": b["pos"][lo:hi].copy(), "l_seq": b["l_seq"][lo:hi].copy(),
            "cig_off": b["cig_off"][lo:hi + 1] - c0, "cigar": b["cigar"][c0:c1].copy(),
            "seq_off": b["seq_off"][lo:hi + 1] - s0, "seq": b["seq"][s0:s1].copy(),
            "qual_off": b["qual_off"][lo:hi + 1] - q0, "qual": b["qual"][q0:q1].copy()}


def batch_args(b):
    """Positional arguments of BaseCounter.add_reads."""
    return (b["tid"], b["pos"], b["cig_off"], b["cigar"], b["l_seq"], b["seq_off"], b["seq"], b["qual_off"],
            b["qual"])


def n_reads(b):
    return len(b["tid"])


# ------------------------------------------------------------------- counts

def read_events(b, i, min_baseq=0):
    """(rpos int64 [k], channel int64 [k]) of read i: one entry per count."""
    words = b["cigar"][int(b["cig_off"][i]):int(b["cig_off"][i + 1])]
    l = int(b["l_seq"][i])
    so, qo = int(b["seq_off"][i]), int(b["qual_off"][i])
    codes = np.zeros(l, np.int64)
    if l:
        by = b["seq"][so:so + (l + 1) // 2].astype(np.int64)
        both = np.stack([by >> 4, by & 15], axis=1).reshape(-1)
        codes = both[:l]
    quals = b["qual"][qo:qo + l].astype(np.int64)
    test = min_baseq > 0 and not (l > 0 and quals[0] == 0xFF)
    chan = np.array(CHANNEL_OF_CODE, np.int64)[codes]
    rp, q = int(b["pos"][i]), 0
    pos_out, ch_out = [], []
    for w in words:
        op, n = int(w) & 15, int(w) >> 4
        if op in (0, 7, 8):
            r = np.arange(rp, rp + n, dtype=np.int64)
            c = chan[q:q + n]
            if test:
                keep = quals[q:q + n] >= min_baseq
                r, c = r[keep], c[keep]
            pos_out.append(r)
            ch_out.append(c)
            rp += n
            q += n
        elif op == 2:
            pos_out.append(np.arange(rp, rp + n, dtype=np.int64))
            ch_out.append(np.full(n, DEL, np.int64))
            rp += n
        elif op == 3:
            rp += n
        elif op in (1, 4):
            q += n
    if not pos_out:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(pos_out), np.concatenate(ch_out)


def seg_offsets(starts, ends):
    off = np.zeros(len(starts) + 1, np.int64)
    off[1:] = np.cumsum(np.asarray(ends, np.int64) - np.asarray(starts, np.int64))
    return off


def counts_model(batches, tids, starts, ends, min_baseq=0):
    """(seg_off [S + 1], planes uint32 [6, N]) of the reads of the batches."""
    if isinstance(batches, dict):
        batches = [batches]
    seg_off = seg_offsets(starts, ends)
    planes = np.zeros((6, int(seg_off[-1])), np.int64)
    ev_t, ev_p, ev_c = [], [], []
    for b in batches:
        for i in range(n_reads(b)):
            p, c = read_events(b, i, min_baseq)
            ev_t.append(np.full(len(p), int(b["tid"][i]), np.int64))
            ev_p.append(p)
            ev_c.append(c)
    if ev_p:
        et, ep, ec = np.concatenate(ev_t), np.concatenate(ev_p), np.concatenate(ev_c)
        for s in range(len(tids)):
            m = (et == int(tids[s])) & (ep >= int(starts[s])) & (ep < int(ends[s]))
            np.add.at(planes, (ec[m], int(seg_off[s]) + ep[m] - int(starts[s])), 1)
    return seg_off, planes.astype(np.uint32)


def int32_edge_case(P, seed=0):
    """One read set at the edge of the int32 positions, for the tests of the
    counts, sites, consensus and insertions (P: the tile size).  On tid 1:
    short reads with pos in [2^31 - 3P, 2^31 - 1] (a 1M read at 2^31 - 1
    among them), reads whose reference end crosses 2^31, three reads at
    2 * 10^9 that skip 7 * (2^28 - 1) positions (their ends lie below 2^32)
    and insertions anchored at 2^31 - 2, 2^31 - 1, 2^31 and on the last
    position of a tile and the one after it.  On tids 0 and 2: ordinary reads
    near position 0.  Returns (reads sorted by (tid, pos), segments, the same
    segments in scrambled order, k: the reads [0, k) lie below (1, 2^31 - P))."""
    rng = np.random.default_rng(seed)
    H, t = 1 << 31, 1

    def rd(tid, pos, cigar, p_n=.04):
        n = query_length(cigar_words(cigar))
        return (tid, int(pos), cigar, "".join(rng.choice(list("ACGTN"), size=n, p=[(1 - p_n) / 4] * 4 + [p_n])), 30)

    seg_a = (t, H - 2 * P - 3, H + P + 5)             # the first segment: its tiles start at multiples of P from it
    reads = [rd(t, p, "40M") for p in rng.integers(H - 3 * P, H - 39, size=60)]
    reads += [rd(t, p, "30M2D8M") for p in rng.integers(H - 3 * P, H - 39, size=20)]
    reads += [rd(t, H - 1, "1M"), rd(t, H - 1, "1M"), rd(t, H - 1, "1D"), rd(t, H - 1, "30M"), rd(t, H - 20, "60M"),
              rd(t, H - 50, "100M"), rd(t, H - 50, "40M5D55M"), rd(t, H - 2 * P - 40, "50M")]
    skip = "".join(["%dN" % ((1 << 28) - 1)] * 7)
    far = [rd(t, 2_000_000_000, "10M" + skip + "10M"), rd(t, 2_000_000_003, "10M" + skip + "4M3I6M", 0),
           rd(t, 2_000_000_005, "6M2I4M" + skip + "5M1D5M")]                 # (no N in the insertion: an allele)
    reads += far
    far_end = max(r[1] + ref_span(cigar_words(r[2])) for r in far)
    assert H + (1 << 30) < far_end < (1 << 32)
    for a in (H - 2, H - 1, H, seg_a[1] + P - 1, seg_a[1] + P, seg_a[1] + 2 * P - 1, seg_a[1] + 2 * P):
        for _ in range(3):
            n = int(rng.integers(1, 3))
            reads.append(rd(t, a - 4, "5M%dI5M" % n))
        reads.append(rd(t, a - 2, "3M2I"))             # a trailing insertion: the anchor is the read's last position
    for tid in (0, 2):
        for p in rng.integers(0, 300, size=40):
            reads.append(rd(tid, p, str(rng.choice(["30M", "10M2I10M", "12M3D9M", "5S20M", "8M1I8M"]))))
    reads.sort(key=lambda r: (r[0], r[1]))
    assert max(r[1] for r in reads) == H - 1
    segs = [seg_a, (t, far_end - P - 35, far_end + 5), (t, H - 1, H), (0, 0, 400), (2, 3, 350)]
    k = sum(1 for r in reads if (r[0], r[1]) < (t, H - P))
    return reads, segs, [segs[i] for i in (3, 1, 4, 0, 2)], k


def counts_loop(batches, tids, starts, ends, min_baseq=0):
    """The same, as a literal per-read, per-base loop (an N op moves the
    reference cursor in one step: a read may skip 2^31 positions)."""
    if isinstance(batches, dict):
        batches = [batches]
    seg_off = seg_offsets(starts, ends)
    planes = np.zeros((6, int(seg_off[-1])), np.uint32)

    def count(tid, p, ch):
        for s in range(len(tids)):
            if int(tids[s]) == tid and int(starts[s]) <= p < int(ends[s]):
                planes[ch, int(seg_off[s]) + p - int(starts[s])] += 1

    for b in batches:
        for i in range(n_reads(b)):
            tid, rp, q, l = int(b["tid"][i]), int(b["pos"][i]), 0, int(b["l_seq"][i])
            so, qo = int(b["seq_off"][i]), int(b["qual_off"][i])
            absent = l > 0 and int(b["qual"][qo]) == 0xFF
            for w in b["cigar"][int(b["cig_off"][i]):int(b["cig_off"][i + 1])]:
                op, n = OPS[int(w) & 15] if (int(w) & 15) < 9 else "?", int(w) >> 4
                if op == "N":
                    rp += n
                    continue
                for _ in range(n):
                    if op in "M=X":
                        byte = int(b["seq"][so + q // 2])
                        code = byte & 15 if q & 1 else byte >> 4
                        ch = {1: A, 2: C, 4: G, 8: T}.get(code, N)
                        if min_baseq <= 0 or absent or int(b["qual"][qo + q]) >= min_baseq:
                            count(tid, rp, ch)
                        rp += 1
                        q += 1
                    elif op == "D":
                        count(tid, rp, DEL)
                        rp += 1
                    elif op in "IS":
                        q += 1
    return seg_off, planes


# -------------------------------------------------------------------- sites

def sites_model(planes, seg_off, starts, min_depth=1, min_count=1, min_ppm=0, ref=None):
    """(site_first [S + 1], site_pos int64, site_counts uint32 [n, 6])."""
    planes = np.asarray(planes)
    n = planes.shape[1]
    al = planes[[A, C, G, T, DEL]].astype(np.int64)
    depth = al.sum(axis=0)
    base = np.argmax(al, axis=0) if n else np.zeros(0, np.int64)      # the first maximum: the lowest channel
    if ref is not None:
        ref = np.asarray(ref, np.int64)
        base = np.where(ref < 4, ref, base)
    others = al.copy()
    if n:
        others[base, np.arange(n)] = -1
    alt = others.max(axis=0) if n else np.zeros(0, np.int64)
    is_site = (depth >= min_depth) & (alt >= min_count) & (alt * 1000000 >= min_ppm * depth)
    idx = np.flatnonzero(is_site)
    first = np.searchsorted(idx, np.asarray(seg_off, np.int64)).astype(np.int64)
    pos = np.zeros(len(idx), np.int64)
    for s in range(len(starts)):
        a, b = int(first[s]), int(first[s + 1])
        pos[a:b] = idx[a:b] - int(seg_off[s]) + int(starts[s])
    return first, pos, planes[:, idx].T.astype(np.uint32).reshape(-1, 6)


# ---------------------------------------------------------------- BAM reader

def read_bam(path):
    """Every record of a BAM as a dict: tid, pos, mapq, flag, l_seq, cigar
    (uint32 words, the CG:B,I placeholder resolved), seq (packed bytes), qual."""
    with gzip.open(path, "rb") as fh:
        d = fh.read()
    assert d[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", d, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", d, o)
    o += 4
    names, lengths = [], []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", d, o)
        names.append(d[o + 4:o + 4 + l_name].split(b"\0")[0].decode())
        lengths.append(struct.unpack_from("<i", d, o + 4 + l_name)[0])
        o += 8 + l_name
    recs = []
    while o + 4 <= len(d):
        bs, = struct.unpack_from("<i", d, o)
        r = o + 4
        tid, pos, l_name, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", d, r)
        c = r + 32 + l_name
        words = np.frombuffer(d, "<u4", n_cig, c).astype(np.uint32)
        s = c + 4 * n_cig
        seq = d[s:s + (l_seq + 1) // 2]
        qual = d[s + (l_seq + 1) // 2:s + (l_seq + 1) // 2 + l_seq]
        aux = s + (l_seq + 1) // 2 + l_seq
        if n_cig == 2 and int(words[0]) == ((l_seq << 4) | 4) and (int(words[1]) & 15) == 3:
            cg = _find_cg(d, aux, r + bs)
            if cg is not None:
                words = cg
        recs.append({"tid": tid, "pos": pos, "mapq": mapq, "flag": flag, "l_seq": l_seq, "cigar": words,
                     "seq": seq, "qual": qual})
        o = r + bs
    return names, lengths, recs


def _find_cg(d, p, end):
    size = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    while p + 3 <= end:
        tag, ty = d[p:p + 2], chr(d[p + 2])
        p += 3
        if ty in size:
            p += size[ty]
        elif ty in "ZH":
            p = d.index(b"\0", p) + 1
        elif ty == "B":
            sub, cnt = chr(d[p]), struct.unpack_from("<I", d, p + 1)[0]
            p += 5
            if tag == b"CG" and sub == "I":
                return np.frombuffer(d, "<u4", cnt, p).astype(np.uint32)
            p += size[sub] * cnt
        else:
            raise ValueError("bad aux type %r" % ty)
    return None


def kept_reads(path, flag_filter=FLAG_FILTER, min_mapq=0):
    """(names, lengths, batch, counts): the kept records of the file as one
    batch with every read's bases on a 4-byte boundary, and the counts
    records / kept (past the filters) / no_seq / bad_cigar (kept but skipped;
    the batch holds kept - no_seq - bad_cigar reads)."""
    names, lengths, recs = read_bam(path)
    counts = {"records": len(recs), "kept": 0, "no_seq": 0, "bad_cigar": 0}
    tid, pos, ls, cig, cig_off, seq, seq_off, qual, qual_off = [], [], [], [], [0], bytearray(), [0], bytearray(), [0]
    last = None
    for r in recs:
        if r["tid"] < 0 or (r["flag"] & flag_filter) or r["mapq"] < min_mapq:
            continue
        counts["kept"] += 1
        if r["l_seq"] == 0:
            counts["no_seq"] += 1
            continue
        if query_length(r["cigar"]) != r["l_seq"]:
            counts["bad_cigar"] += 1
            continue
        if last is not None and (r["tid"], r["pos"]) < last:
            raise ValueError("unsorted")
        last = (r["tid"], r["pos"])
        tid.append(r["tid"])
        pos.append(r["pos"])
        ls.append(r["l_seq"])
        cig.append(r["cigar"])
        cig_off.append(cig_off[-1] + len(r["cigar"]))
        seq.extend(r["seq"])
        seq.extend(b"\0" * (-len(seq) % 4))
        seq_off.append(len(seq))
        qual.extend(r["qual"])
        qual_off.append(len(qual))
    batch = {"tid": np.array(tid, np.int32), "pos": np.array(pos, np.int32), "l_seq": np.array(ls, np.int32),
             "cig_off": np.array(cig_off, np.int64),
             "cigar": np.concatenate(cig + [np.zeros(0, np.uint32)]).astype(np.uint32),
             "seq_off": np.array(seq_off, np.int64), "seq": np.frombuffer(bytes(seq), np.uint8).copy(),
             "qual_off": np.array(qual_off, np.int64), "qual": np.frombuffer(bytes(qual), np.uint8).copy()}
    return names, lengths, batch, counts


# -------------------------------------------------------------------- table

def read_fasta(path):
    """{first word of the header: sequence string} of a plain or gzip FASTA."""
    with open(path, "rb") as fh:
        gz = fh.read(2) == b"\x1f\x8b"
    with (gzip.open if gz else open)(path, "rt") as fh:
        out, name = {}, None
        for line in fh:
            if line.startswith(">"):
                name = line[1:].split()[0]
                out[name] = []
            elif name is not None:
                out[name].append(line.strip())
    return {k: "".join(v) for k, v in out.items()}


def table(name_of, rows, fasta=None):
    """The `bases` table: rows of (tid, 0-based pos, six counts)."""
    out = ["contig\tpos\tref\tdepth\tA\tC\tG\tT\tN\tDEL\n"]
    for tid, p, c in rows:
        ref = "."
        if fasta is not None:
            s = fasta.get(name_of[tid], "")
            ref = s[p].upper() if p < len(s) else "N"
        c = [int(x) for x in c]
        out.append("%s\t%d\t%s\t%d\t%s\n" % (name_of[tid], p + 1, ref, c[A] + c[C] + c[G] + c[T] + c[DEL],
                                             "\t".join(str(x) for x in c)))
    return "".join(out)
