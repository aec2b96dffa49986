"""Model of the insertion alleles (include/metacov_amd.h, "Insertion
alleles"), pure Python / numpy, restated from the contract and not from the
library's code:

walk       bases_model's: from rpos = pos, qpos = 0
event      an I op of length L >= 1 met at rpos > pos (M/=/X/D/N ops of at
           least one reference position precede it) is an event at anchor
           p = rpos - 1; a leading insertion is ignored, a trailing one
           counts, two I ops at one anchor are two events; no quality test
allele     L <= 32 and all L bases among nt16 1/2/4/8: (len, code) = (L,
           sum b_j 4^(L-1-j)), A C G T = 0..3; otherwise OTHER = (0, 0) with
           other = 1
planes     an event belongs to every plane index i whose segment holds p
table      rows (i, len, code, other, count) sorted by (i, other, len, code),
           unique; first[s] = rows with i < seg_off[s]
filter     depth = A+C+G+T+DEL at i; depth >= min_depth, count >= min_count,
           count * 10^6 >= min_ppm * depth
consensus  at i not LOW: top = the row that is not OTHER with the highest
           count (ties: shorter len, then smaller code); if qualifies(count)
           its letters follow i's letter in the compact output (where i is
           DEL: in that letter's place); length = positions - deleted +
           inserted; inserted[s] = (insertions called, bases inserted)
"""
import numpy as np

from . import bases_model as bm
from . import consensus_model as cm

MAX_LEN = 32
BASE_OF_CODE = {1: 0, 2: 1, 4: 2, 8: 3}
HEADER = "contig\tpos\tdepth\tcount\tlen\tseq\n"
SUMMARY_HEADER = cm.SUMMARY_HEADER[:-1] + "\tinsertions\tinserted\n"


def encode(seq):
    """'ACG' -> its code."""
    c = 0
    for ch in seq:
        c = c * 4 + "ACGT".index(ch)
    return c


def decode(length, code):
    return "".join("ACGT"[(int(code) >> (2 * (int(length) - 1 - j))) & 3] for j in range(int(length)))


def _codes(b, i):
    l = int(b["l_seq"][i])
    so = int(b["seq_off"][i])
    by = b["seq"][so:so + (l + 1) // 2].astype(np.int64)
    return np.stack([by >> 4, by & 15], axis=1).reshape(-1)[:l]


def read_insertions(b, i):
    """[(anchor, len, code, other)] of read i, ops taken whole (numpy)."""
    words = b["cigar"][int(b["cig_off"][i]):int(b["cig_off"][i + 1])].astype(np.int64)
    ops, lens = words & 15, words >> 4
    ref = np.isin(ops, [0, 2, 3, 7, 8])
    qry = np.isin(ops, [0, 1, 4, 7, 8])
    r_at = int(b["pos"][i]) + np.concatenate([[0], np.cumsum(lens * ref)])[:-1]     # cursor in front of each op
    q_at = np.concatenate([[0], np.cumsum(lens * qry)])[:-1]
    codes = _codes(b, i)
    out = []
    for k in np.flatnonzero((ops == 1) & (lens >= 1) & (r_at > int(b["pos"][i]))):
        n = int(lens[k])
        ins = codes[int(q_at[k]):int(q_at[k]) + n]
        if n <= MAX_LEN and np.isin(ins, [1, 2, 4, 8]).all():
            digits = np.log2(ins).astype(np.int64)
            code = 0
            for d in digits.tolist():
                code = code * 4 + d
            out.append((int(r_at[k]) - 1, n, code, 0))
        else:
            out.append((int(r_at[k]) - 1, 0, 0, 1))
    return out


def read_insertions_loop(b, i):
    """The same by a literal walk, base by base."""
    pos, l = int(b["pos"][i]), int(b["l_seq"][i])
    so = int(b["seq_off"][i])
    rp, q, out = pos, 0, []
    for w in b["cigar"][int(b["cig_off"][i]):int(b["cig_off"][i + 1])]:
        op, n = int(w) & 15, int(w) >> 4
        if op == 1:
            if n >= 1 and rp > pos:
                other, code = n > MAX_LEN, 0
                for j in range(n):
                    if other:
                        break
                    byte = int(b["seq"][so + (q + j) // 2])
                    nt = byte & 15 if (q + j) & 1 else byte >> 4
                    if nt not in BASE_OF_CODE:
                        other = True
                    else:
                        code = code * 4 + BASE_OF_CODE[nt]
                out.append((rp - 1, 0, 0, 1) if other else (rp - 1, n, code, 0))
            q += n
        elif op == 4:
            q += n
        elif op in (0, 7, 8):
            rp += n
            q += n
        elif op in (2, 3):
            rp += n
    assert q == l
    return out


def make_table(rows):
    """rows: iterable of (i, len, code, other, count) -> dict of arrays."""
    rows = list(rows)
    return {"i": np.array([r[0] for r in rows], np.int64), "len": np.array([r[1] for r in rows], np.int32),
            "code": np.array([r[2] for r in rows], np.uint64), "other": np.array([r[3] for r in rows], np.uint8),
            "count": np.array([r[4] for r in rows], np.uint32)}


def table_rows(t):
    return [(int(a), int(b), int(c), int(d), int(e))
            for a, b, c, d, e in zip(t["i"], t["len"], t["code"], t["other"], t["count"])]


def table_model(batches, tids, starts, ends, per_read=read_insertions):
    """The full allele table of the reads of the batches over the segments."""
    if isinstance(batches, dict):
        batches = [batches]
    seg_off = bm.seg_offsets(starts, ends)
    counts = {}
    for b in batches:
        for r in range(bm.n_reads(b)):
            tid = int(b["tid"][r])
            for p, n, code, other in per_read(b, r):
                for s in range(len(tids)):
                    if int(tids[s]) == tid and int(starts[s]) <= p < int(ends[s]):
                        key = (int(seg_off[s]) + p - int(starts[s]), other, n, code)
                        counts[key] = counts.get(key, 0) + 1
    return make_table((i, n, code, other, c) for (i, other, n, code), c in sorted(counts.items()))


def table_loop(batches, tids, starts, ends):
    return table_model(batches, tids, starts, ends, per_read=read_insertions_loop)


def depth_of(planes):
    planes = np.asarray(planes)
    return planes[[bm.A, bm.C, bm.G, bm.T, bm.DEL]].astype(np.int64).sum(axis=0)


def filter_table(t, planes, min_depth=1, min_count=1, min_ppm=0):
    """The rows that pass the sites predicate (Python integers)."""
    depth = depth_of(planes)
    keep = [r for r in table_rows(t)
            if int(depth[r[0]]) >= min_depth and r[4] >= min_count and r[4] * 10 ** 6 >= min_ppm * int(depth[r[0]])]
    return make_table(keep)


def first_of(t, seg_off):
    return np.searchsorted(t["i"], np.asarray(seg_off, np.int64), side="left").astype(np.int64)


def table_bytes(t, seg_off):
    """Every byte the library hands out for the table, for equality tests."""
    return b"".join(np.ascontiguousarray(a).tobytes() for a in
                    (first_of(t, seg_off), t["i"], t["len"], t["code"], t["other"], t["count"]))


def called_insertions(planes, t, min_depth=1, min_count=1, call_ppm=0):
    """{i: sequence} of the insertions the consensus calls."""
    depth = depth_of(planes)
    best = {}
    for i, n, code, other, c in table_rows(t):
        if other:
            continue
        key = (-c, n, code)                      # highest count, then shorter, then smaller code
        if i not in best or key < best[i]:
            best[i] = key
    out = {}
    for i, (negc, n, code) in best.items():
        d, c = int(depth[i]), -negc
        if d < max(min_depth, 1):
            continue                             # LOW
        if c >= max(min_count, 1) and c * 10 ** 6 >= call_ppm * d:
            out[i] = decode(n, code)
    return out


def consensus_model(planes, seg_off, t, min_depth=1, min_count=1, call_ppm=0, **kw):
    """(first [S + 1], summary [S, 8], inserted [S, 2], aligned uint8 [N],
    compact uint8) of the consensus with insertions."""
    first0, summary, aligned, _ = cm.consensus_model(planes, seg_off, min_depth=min_depth, min_count=min_count,
                                                     call_ppm=call_ppm, **kw)
    called = called_insertions(planes, t, min_depth, min_count, call_ppm)
    S = len(seg_off) - 1
    first = np.zeros(S + 1, np.int64)
    inserted = np.zeros((S, 2), np.int64)
    summary = summary.copy()
    parts = []
    for s in range(S):
        seg = []
        for i in range(int(seg_off[s]), int(seg_off[s + 1])):
            if aligned[i] != ord("-"):
                seg.append(chr(aligned[i]))
            if i in called:
                seg.append(called[i])
                inserted[s, 0] += 1
                inserted[s, 1] += len(called[i])
        text = "".join(seg)
        parts.append(text)
        summary[s, cm.COL_LENGTH] += inserted[s, 1]
        assert len(text) == summary[s, cm.COL_LENGTH]
        first[s + 1] = first[s] + len(text)
    return first, summary, inserted, aligned, np.frombuffer("".join(parts).encode(), np.uint8)


def tsv(name_of, tids, starts, seg_off, planes, t, header=True):
    """The `bases --insertions` table of the (filtered) table t."""
    depth = depth_of(planes)
    first = first_of(t, seg_off)
    out = [HEADER] if header else []
    rows = table_rows(t)
    for s in range(len(tids)):
        for i, n, code, other, c in rows[int(first[s]):int(first[s + 1])]:
            out.append("%s\t%d\t%d\t%d\t%d\t%s\n" % (name_of[int(tids[s])], i - int(seg_off[s]) + int(starts[s]) + 1,
                                                   int(depth[i]), c, n, "*" if other else decode(n, code)))
    return "".join(out)


def summary_table(rows):
    """rows: (name, start, end, eight numbers, two numbers)."""
    return SUMMARY_HEADER + "".join("%s\t%d\t%d\t%s\n" % (n, a, b, "\t".join(str(int(v)) for v in list(r) + list(x)))
                                    for n, a, b, r, x in rows)


# ------------------------------------------------------------ cases by hand
# (reads, the rows (i, len, code, other, count) of the full table)
# every case: one segment (0, 100, 200), plane index = position - 100

SEG = [(0, 100, 200)]

HAND = [
    # a leading I (only S / H / I before it) is ignored; the one behind the M counts
    ([(0, 110, "2S3I4M1I2M", "TTAAACCCCGTT", 30)], [(13, 1, encode("G"), 0, 1)]),
    ([(0, 110, "2H1I1I4M", "AACCCC", 30)], []),
    # an I after D and after N: anchored on the last deleted / skipped position
    ([(0, 110, "2M3D2I2M", "AACGTT", 30)], [(14, 2, encode("CG"), 0, 1)]),
    ([(0, 110, "2M5N1I2M", "AATCC", 30)], [(16, 1, encode("T"), 0, 1)]),
    # D first: a reference op precedes the I although no base was read
    ([(0, 110, "2D1I2M", "GAA", 30)], [(11, 1, encode("G"), 0, 1)]),
    # a trailing I before S counts, anchored on the read's last reference position
    ([(0, 110, "4M2I3S", "ACGTCATTT", 30)], [(13, 2, encode("CA"), 0, 1)]),
    # len 1, 32 (callable) and 33 (OTHER)
    ([(0, 120, "1M1I1M", "ATA", 30)], [(20, 1, encode("T"), 0, 1)]),
    ([(0, 120, "1M32I1M", "A" + "ACGT" * 8 + "A", 30)], [(20, 32, encode("ACGT" * 8), 0, 1)]),
    ([(0, 120, "1M33I1M", "A" + "ACGT" * 8 + "AA", 30)], [(20, 0, 0, 1, 1)]),
    ([(0, 120, "1M32I1M", "A" + "T" * 32 + "A", 30)], [(20, 32, 2 ** 64 - 1, 0, 1)]),
    # an N or an M code inside: OTHER; both share the position's one OTHER row
    ([(0, 120, "1M3I1M", "AANAA", 30), (0, 120, "1M2I1M", "AMAA", 30), (0, 120, "1M2I1M", "AAAA", 30)],
     [(20, 2, encode("AA"), 0, 1), (20, 0, 0, 1, 2)]),
    # two I ops of one read at one anchor are two events (here: two alleles, and the same allele twice)
    ([(0, 130, "2M1I2I2M", "AACGTAA", 30)], [(31, 1, encode("C"), 0, 1), (31, 2, encode("GT"), 0, 1)]),
    ([(0, 130, "2M1I1P1I2M", "AACCAA", 30)], [(31, 1, encode("C"), 0, 2)]),
    # qualities never matter, absent ones neither
    ([(0, 130, "2M1I2M", "AACAA", 0), (0, 130, "2M1I2M", "AACAA", None)], [(31, 1, encode("C"), 0, 2)]),
    # anchors outside the segment add nothing: before it, behind it, on another contig; its edges count
    ([(0, 98, "2M1I2M", "AACAA", 30), (0, 99, "2M1I2M", "AAGAA", 30), (0, 198, "2M1I2M", "AATAA", 30),
      (0, 199, "2M1I2M", "AACAA", 30), (1, 150, "2M1I2M", "AACAA", 30)],
     [(0, 1, encode("G"), 0, 1), (99, 1, encode("T"), 0, 1)]),
    # order: (i, other, len, code): shorter first, then by code (lexicographic), OTHER last, counts grouped
    ([(0, 140, "1M2I1M", "ACAA", 30), (0, 140, "1M2I1M", "AACA", 30), (0, 140, "1M1I1M", "ATA", 30),
      (0, 140, "1M1I1M", "ANA", 30), (0, 140, "1M2I1M", "ACAA", 30), (0, 139, "1M3I1M", "ATTTA", 30)],
     [(39, 3, encode("TTT"), 0, 1), (40, 1, encode("T"), 0, 1), (40, 2, encode("AC"), 0, 1), (40, 2, encode("CA"), 0, 2),
      (40, 0, 0, 1, 1)]),
]



# --------------------------------------------------------------- random reads

def random_reads(rng, n, n_ref=2, length=5000, ins_frac=0.05, max_read=120):
    """n sorted reads (tuples for bases_model.make_batch); ins_frac of them
    carry one to three insertions, some long, some with an N inside, some
    leading or trailing, now and then two in a row."""
    reads = []
    for _ in range(n):
        tid = int(rng.integers(0, n_ref))
        pos = int(rng.integers(0, length))
        m = int(rng.integers(1, max_read))
        ops = []
        if rng.random() < 0.2:
            ops.append((4, int(rng.integers(1, 6))))
        if rng.random() < ins_frac:
            k = int(rng.integers(1, 4))
            if rng.random() < 0.2:
                ops.append((1, int(rng.integers(1, 4))))               # leading: ignored
            for j in range(k):
                ops.append((int(rng.choice([0, 7, 8])), int(rng.integers(1, max(2, m // k)))))
                if rng.random() < 0.3:
                    ops.append((int(rng.choice([2, 3])), int(rng.integers(1, 5))))
                ops.append((1, int(rng.choice([1, 1, 2, 2, 3, 5, 32, 33, 40]))))
                if rng.random() < 0.15:
                    ops.append((1, int(rng.integers(1, 3))))           # a second I at the same anchor
            if rng.random() < 0.7:
                ops.append((0, int(rng.integers(1, 20))))
        else:
            ops.append((0, m))
            if rng.random() < 0.2:
                ops.append((2, int(rng.integers(1, 4))))
                ops.append((0, int(rng.integers(1, 20))))
        if rng.random() < 0.2:
            ops.append((4, int(rng.integers(1, 6))))
        q = sum(n_ for op, n_ in ops if op in bm.QUERY_OPS)
        alphabet = "ACGT" if rng.random() < 0.8 else "ACGTNM"
        # few distinct alleles per anchor: short insertions from a two-letter alphabet half of the time
        if rng.random() < 0.5:
            alphabet = "AC"
        bases = "".join(rng.choice(list(alphabet), q).tolist())
        reads.append((tid, pos, ops, bases, int(rng.integers(0, 41))))
    reads.sort(key=lambda r: (r[0], r[1]))
    return reads
