"""Per-allele quality sums on the GPU (csrc/bases.hip, the quality
instantiation of the pileup kernel and the quality sites kernels) against
tests/quality_model.py: exact equality of the counts and both sum sets, the
sites and the CLI's bytes.  Shapes are a few tiles at most; P (the tile) and Q
(the positions one workgroup of the quality kernel owns) come from the
library."""
import ctypes
import os

import numpy as np
import pytest
from click.testing import CliRunner

from metacov_amd import _lib
from metacov_amd import bases as mb
from tests import bases_model as bm
from tests import quality_model as qm
from tests.bases_model import A, C, G, T, N, DEL

pytestmark = pytest.mark.gpu

N_REF = 4
GOLDENS = ["bbmap.sorted.bam", "synth_edge.bam", "synth_exp.bam", "synth_exp_noseq.bam", "synth_longcigar.bam",
           "synth_multi.bam"]
CLI_BASEQ, CLI_MAPQ = 36, 40             # thresholds of the CLI run: they keep under half of the plain sites


@pytest.fixture(scope="module")
def bc(lib_built):
    h = mb.BaseCounter(N_REF, 0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def P(lib_built):
    return mb.dims()


@pytest.fixture(scope="module")
def Q(lib_built, P):
    q, group = mb.quality_dims()
    assert P % q == 0 and q % 4 == 0 and group == 65535
    return q


def arrays(segs):
    return tuple(np.array(x, np.int64) for x in zip(*segs))


def run(bc, batches, mapqs, segs, min_baseq=0, quality=True):
    """(total, bq, mq) of a quality-tracking counter, or (total, None, None)."""
    tids, starts, ends = arrays(segs)
    n = bc.begin(tids, starts, ends, min_baseq=min_baseq, quality=quality)
    for b, m in zip(batches, mapqs):
        bc.add_reads(*bm.batch_args(b), mapq=m if quality else None)
    total = bc.counts()
    assert total.dtype == np.uint32 and total.shape == (6, n)
    if not quality:
        return total, None, None
    bq, mq = bc.quality()
    assert bq.dtype == np.uint32 and bq.shape == (6, n) and mq.dtype == np.uint32 and mq.shape == (6, n)
    return total, bq, mq


def same(got, want, what):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: first difference at (channel, index) %s: got %d, want %d" % (
        what, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def check(bc, batches, mapqs, segs, min_baseq=0, loop=False):
    """The counts and both sum sets against the model, the counts against a
    counter without tracking fed the same reads."""
    if isinstance(batches, dict):
        batches, mapqs = [batches], [mapqs]
    tids, starts, ends = arrays(segs)
    total, bq, mq = run(bc, batches, mapqs, segs, min_baseq)
    _, want_total, want_bq, want_mq = qm.counts_model(batches, mapqs, tids, starts, ends, min_baseq, loop=loop)
    same(total, want_total, "total")
    same(bq, want_bq, "bq")
    same(mq, want_mq, "mq")
    assert bq[DEL].sum() == 0
    plain, _, _ = run(bc, batches, mapqs, segs, min_baseq, quality=False)
    assert np.array_equal(plain, total)
    return total, bq, mq


def random_quals(rng, k, absent=.15):
    """None (absent) or k bytes from 0 up to 254."""
    return None if rng.random() < absent else [int(x) for x in rng.integers(0, 255, size=k)]


def random_mapq(rng, n):
    """Bytes over 0..255 with both ends present."""
    m = rng.integers(0, 256, size=n).astype(np.uint8)
    m[rng.choice(n, size=2, replace=False)] = [0, 255]
    return m


# ------------------------------------------------------------- 1. random reads

CIGARS = ["40M", "12M3I20M", "15M4D15M", "10M30N12M", "5S25M", "25M6S", "3H20M2H", "8=2X8=",
          "2H3S5M2I4M3D6M7N2=1X1P2M4S", "1M", "60M", "7M1D7M1I7M"]


@pytest.fixture(scope="module")
def random_reads(P):
    """About 400 reads over 3 contigs of more than one tile, with their mapq."""
    rng = np.random.default_rng(31)
    lengths = [2 * P + 77, P - 3, 300]
    reads = []
    for _ in range(400):
        t = int(rng.choice(3, p=[.6, .3, .1]))
        c = str(rng.choice(CIGARS))
        k = bm.query_length(bm.cigar_words(c))
        reads.append((t, int(rng.integers(0, lengths[t] - 20)), c,
                      "".join(rng.choice(list("ACGTN"), size=k, p=[.24, .24, .24, .24, .04])), random_quals(rng, k)))
    reads.sort(key=lambda r: (r[0], r[1]))
    b = bm.make_batch(reads)
    assert set("".join(CIGARS)) >= set("MIDNSH=X")
    return b, random_mapq(rng, len(reads)), [(t, 0, L) for t, L in enumerate(lengths)]


@pytest.mark.parametrize("min_baseq", [0, 20])
def test_random_reads(bc, random_reads, min_baseq):
    b, mapq, segs = random_reads
    first = [int(b["qual"][int(b["qual_off"][i])]) for i in range(bm.n_reads(b))]
    assert 20 < sum(f == 0xFF for f in first) < 120 and int(b["qual"].min()) == 0 and 254 in b["qual"]
    assert int(mapq.min()) == 0 and int(mapq.max()) == 255
    total, bq, mq = check(bc, b, mapq, segs, min_baseq)
    assert bq.sum() > 0 and mq[DEL].sum() > 0 and total[DEL].sum() > 0


# ---------------------------------------------------- 2. tile and segment edges

def test_tile_and_segment_edges(bc, P, Q):
    rng = np.random.default_rng(32)

    def rd(t, pos, cigar):
        k = bm.query_length(bm.cigar_words(cigar))
        return (t, pos, cigar, "".join(rng.choice(list("ACGT"), size=k)), random_quals(rng, k, .1))

    lengths = [P - 1, P, P + 1, 2 * P + 1]
    reads = []
    for t, L in enumerate(lengths):
        for edge in range(Q, L + 1, Q):                         # every edge between two workgroups' positions
            reads += [rd(t, edge - 30, "60M"), rd(t, edge - 1, "1M"), rd(t, edge, "1M"), rd(t, edge - 1, "2M"),
                      rd(t, edge - 20, "15M10D15M"), rd(t, edge - 10, "10M5I10M"), rd(t, edge - 40, "40M")]
        reads += [rd(t, 0, "30M"), rd(t, L - 10, "30M"), rd(t, L - 1, "1M")]
    # reads whose only overlap with a workgroup's positions is a deletion: three positions, and all of them
    reads += [rd(3, P - 10, "10M3D"), rd(3, P - 5, "5M%dD5M" % Q), rd(3, Q - 5, "5M%dD5M" % P)]
    reads.sort(key=lambda r: (r[0], r[1]))
    b = bm.make_batch(reads)
    mapq = random_mapq(rng, len(reads))
    # segments at plane offsets 1, 2 and 3 past a multiple of four (lead != 0), an overlapping, a duplicated
    # and an empty one
    segs = [(0, 0, P - 1), (1, 0, P), (2, 0, P + 1), (3, 0, 2 * P + 1), (3, 5, P + 6), (1, 9, 9), (3, 0, 2 * P + 1),
            (2, 3, Q + 8), (3, P - 1, P + 1)]
    off = bm.seg_offsets([s[1] for s in segs], [s[2] for s in segs])
    assert [int(o) & 3 for o in off[1:8]] == [3, 3, 0, 1, 2, 2, 3] and off[5] == off[6]
    total, bq, mq = check(bc, b, mapq, segs)
    dup = slice(int(off[6]), int(off[7]))
    for v in (total, bq, mq):
        assert np.array_equal(v[:, int(off[3]):int(off[4])], v[:, dup])
    third = slice(int(off[3]) + P, int(off[3]) + P + Q)         # contig 3's third run of Q positions
    assert total[DEL, third].min() >= 1 and mq[DEL, third].max() > 0


# -------------------------------------------------------- 3. batch independence

def test_batch_independence(bc, random_reads):
    b, mapq, segs = random_reads
    n = bm.n_reads(b)
    want = None
    for parts in (1, 10, n):
        cuts = [n * k // parts for k in range(parts + 1)]
        batches = [bm.slice_batch(b, x, y) for x, y in zip(cuts, cuts[1:])]
        got = run(bc, batches, [mapq[x:y] for x, y in zip(cuts, cuts[1:])], segs, 20)
        if want is None:
            want = got
            assert want[1].sum() > 0 and want[2].sum() > 0
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), parts


# ------------------------------------------------------- 4. field-width boundary

def one_base_reads(tid, piles):
    """Reads `1M` on contig tid: piles of (pos, n, nt16 code, quality, mapq),
    by ascending pos; (batch, mapq)."""
    n = sum(p[1] for p in piles)
    ar = np.arange(n + 1, dtype=np.int64)
    rep = lambda k, dt: np.concatenate([np.full(p[1], p[k], dt) for p in piles])
    b = {"tid": np.full(n, tid, np.int32), "pos": rep(0, np.int32), "l_seq": np.ones(n, np.int32), "cig_off": ar,
         "cigar": np.full(n, (1 << 4) | 0, np.uint32), "seq_off": ar, "seq": (rep(2, np.uint8) << 4).astype(np.uint8),
         "qual_off": ar, "qual": rep(3, np.uint8)}
    return b, rep(4, np.uint8)


def test_field_width_boundary(bc):
    """One-base reads with quality 254 and MAPQ 255 piled on one position: a
    group of 65535 reads fills the 16-bit count and nearly the two 24-bit sums
    of a packed LDS cell; one read more would carry into the next field, and
    the cell's last field into nothing.  The neighbouring positions carry small
    piles, so the reads a workgroup looks at split into groups inside the pile."""
    sizes = [65535, 65536, 70003]
    batches, mapqs = [], []
    want = [np.zeros((6, 24), np.uint32) for _ in range(3)]
    for t, n in enumerate(sizes):
        piles = [(4, 3, 2, 7, 9), (5, n, 1, 254, 255), (6, 2, 8, 254, 255), (7, 1, 1, 0, 0)]
        b, m = one_base_reads(t, piles)
        batches.append(b)
        mapqs.append(m)
        for pos, k, code, q, mq in piles:
            ch = {1: A, 2: C, 4: G, 8: T}[code]
            want[0][ch, 8 * t + pos] = k
            want[1][ch, 8 * t + pos] = k * q
            want[2][ch, 8 * t + pos] = k * mq
    assert [bm.n_reads(b) for b in batches] == [n + 6 for n in sizes]
    segs = [(0, 0, 8), (1, 0, 8), (2, 0, 8)]
    total, bq, mq = run(bc, batches, mapqs, segs)
    same(total, want[0], "total")
    same(bq, want[1], "bq")
    same(mq, want[2], "mq")
    assert bq[A, 5] == 65535 * 254 and mq[A, 21] == 70003 * 255
    plain, _, _ = run(bc, batches, mapqs, segs, quality=False)
    assert np.array_equal(plain, total)
    # the same piles in one batch per contig half: the groups start elsewhere, the sums stay
    halves = [bm.slice_batch(b, x, y) for b in batches for x, y in ((0, 40000), (40000, bm.n_reads(b)))]
    hm = [m[x:y] for m, b in zip(mapqs, batches) for x, y in ((0, 40000), (40000, bm.n_reads(b)))]
    again = run(bc, halves, hm, segs)
    assert all(np.array_equal(g, w) for g, w in zip(again, (total, bq, mq)))


# ------------------------------------------------------------------ 5. int32 edge

def test_int32_edge(bc, P):
    reads, segs, _, k = bm.int32_edge_case(P)
    rng = np.random.default_rng(35)
    reads = [r[:4] + (random_quals(rng, len(r[3])),) for r in reads]
    b = bm.make_batch(reads)
    n = bm.n_reads(b)
    mapq = random_mapq(rng, n)
    assert int(b["pos"].max()) == (1 << 31) - 1 and 0 < k < n
    batches = [bm.slice_batch(b, 0, k), bm.slice_batch(b, k, n)]
    total, bq, mq = check(bc, batches, [mapq[:k], mapq[k:]], segs, loop=True)
    assert bq.sum() > 0 and mq.sum() > 0


# ------------------------------------------------------- 6. sites on crafted planes

BIG = 16843010                                  # the least count whose sums may reach 2^32 - 1 (255 x BIG >= 2^32 - 1)
FULL = (1 << 32) - 1


def crafted_planes(P, Q, segs):
    """Counts, both sum sets and a reference plane over the segments: random
    background without alternative alleles, then the rows of interest (with
    thresholds 20 and 30 in mind)."""
    rng = np.random.default_rng(36)
    off = bm.seg_offsets([s[1] for s in segs], [s[2] for s in segs])
    n = int(off[-1])
    total, bq, mq = (np.zeros((6, n), np.uint32) for _ in range(3))
    total[A] = rng.integers(0, 40, size=n)                       # one allele only: no site
    bq[A] = rng.integers(0, 256, size=n) * total[A]
    mq[A] = rng.integers(0, 256, size=n) * total[A]
    total[N] = rng.integers(0, 3, size=n)
    bq[N] = 40 * total[N]
    mq[N] = 60 * total[N]
    ref = np.full(n, 4, np.uint8)
    rows = {}

    def put(name, i, t, b, m, rf=4):
        total[:, i], bq[:, i], mq[:, i], ref[i] = t, b, m, rf
        rows[name] = i

    #                      A   C  G  T  N DEL
    put("at", 10, [30, 8, 0, 0, 0, 0], [900, 160, 0, 0, 0, 0], [1800, 240, 0, 0, 0, 0])        # bq = 20 a, mq = 30 a
    put("bq_below", 11, [30, 8, 0, 0, 0, 0], [900, 159, 0, 0, 0, 0], [1800, 240, 0, 0, 0, 0])
    put("mq_below", 12, [30, 8, 0, 0, 0, 0], [900, 160, 0, 0, 0, 0], [1800, 239, 0, 0, 0, 0])
    put("weaker_ok", 13, [30, 8, 0, 4, 1, 0], [900, 0, 0, 80, 0, 0], [1800, 2040, 0, 120, 0, 0])  # C fails bq, T passes
    put("del_only", 14, [30, 0, 0, 0, 0, 9], [900, 0, 0, 0, 0, 0], [1800, 0, 0, 0, 0, 270])    # DEL: mq = 30 a, no bq
    put("del_mq_below", 15, [30, 0, 0, 0, 0, 9], [900, 0, 0, 0, 0, 0], [1800, 0, 0, 0, 0, 269])
    put("ref_minority", 16, [30, 6, 0, 0, 0, 0], [600, 114, 0, 0, 0, 0], [900, 180, 0, 0, 0, 0], 1)     # ref C: alt A
    put("full", 17, [20000000, BIG, 0, 0, 0, 0], [FULL, FULL, 0, 0, 0, 0], [FULL, FULL, 0, 0, 0, 0])
    put("full_del", 18, [20000000, 0, 0, 0, 0, BIG], [FULL, 0, 0, 0, 0, 0], [FULL, 0, 0, 0, 0, FULL])
    good = ([20, 0, 6, 0, 0, 0], [400, 0, 120, 0, 0, 0], [600, 0, 180, 0, 0, 0])
    places = [Q - 1, Q, P - 1, P, 2 * P - 1, 2 * P, int(off[1]), int(off[1]) + P - 2, int(off[1]) + P - 1,
              int(off[2]) - 1, int(off[2]), int(off[2]) + 17, n - 1]
    assert len(set(places)) == len(places) and min(places) > 100 and max(places) == n - 1
    for k, i in enumerate(places):                              # tile edges, segment ends, unaligned segments
        put("place%d" % k, i, *good)
    assert (bq.astype(np.int64) <= 255 * total.astype(np.int64)).all() and bq[DEL].sum() == 0
    assert (mq.astype(np.int64) <= 255 * total.astype(np.int64)).all()
    return off, total, bq, mq, ref, rows, places


def _plane_index(sites, off, starts):
    """Plane indices of the sites."""
    out = np.zeros(len(sites), np.int64)
    for s in range(len(starts)):
        a, b = int(sites.first[s]), int(sites.first[s + 1])
        out[a:b] = sites.pos[a:b] - int(starts[s]) + int(off[s])
    return out


def test_sites_on_crafted_planes(bc, P, Q):
    segs = [(0, 0, 2 * P + 1), (1, 100, 100 + P + 2), (2, 7, 7 + 50)]        # the later ones start at offsets 1 and 3
    tids, starts, ends = arrays(segs)
    off, total, bq, mq, ref, rows, places = crafted_planes(P, Q, segs)
    assert [int(o) & 3 for o in off[1:3]] == [1, 3]
    bc.begin(tids, starts, ends, quality=True)
    bc.set_counts(0, total, bq=bq, mq=mq)
    got_bq, got_mq = bc.quality()
    assert np.array_equal(bc.counts(), total) and np.array_equal(got_bq, bq) and np.array_equal(got_mq, mq)
    args = (4, 3, 50000)
    with mb.BaseCounter(N_REF, 0) as plain:                     # both thresholds 0: the plain list
        plain.begin(tids, starts, ends)
        plain.set_counts(0, total)
        for r in (None, ref):
            want = plain.sites(*args, ref=r)
            got = bc.sites(*args, ref=r)
            assert want.bq_sums is None and want.mq_sums is None and len(want) > len(places)
            assert np.array_equal(got.first, want.first) and np.array_equal(got.pos, want.pos)
            assert np.array_equal(got.counts, want.counts)
            idx = _plane_index(got, off, starts)
            assert np.array_equal(got.bq_sums, bq[:, idx].T) and np.array_equal(got.mq_sums, mq[:, idx].T)
    seen = {}
    for th in ((20, 30), (20, 0), (0, 30), (21, 30), (20, 31), (255, 30), (254, 254), (255, 255), (0, 255)):
        for r in (None, ref):
            got = bc.sites(*args, ref=r, min_alt_baseq=th[0], min_alt_mapq=th[1])
            first, pos, cnt, sb, sq = qm.sites_model(total, bq, mq, off, starts, *args, th[0], th[1], r)
            assert np.array_equal(got.first, first) and np.array_equal(got.pos, pos), (th, r is not None)
            assert np.array_equal(got.counts, cnt) and np.array_equal(got.bq_sums, sb)
            assert np.array_equal(got.mq_sums, sq)
            assert got.bq_sums.dtype == np.uint32 and got.mq_sums.shape == (len(got), 6)
            seen[th, r is not None] = set(_plane_index(got, off, starts).tolist())
    s = seen[(20, 30), True]
    assert rows["at"] in s and rows["bq_below"] not in s and rows["mq_below"] not in s and rows["weaker_ok"] in s
    assert rows["del_only"] in s and rows["del_mq_below"] not in s and rows["ref_minority"] in s
    assert rows["ref_minority"] not in seen[(20, 30), False]    # without ref A is the base allele there
    assert rows["bq_below"] in seen[(0, 30), True] and rows["mq_below"] in seen[(20, 0), True]
    assert set(places) <= s and not set(places) & seen[(21, 30), True] and not set(places) & seen[(20, 31), True]
    # DEL as the only alternative allele is exempt from the baseq threshold
    assert rows["del_only"] in seen[(255, 30), True] and rows["at"] not in seen[(255, 30), True]
    # sums of 2^32 - 1 over BIG reads: a mean of 254.99...; 255 x BIG does not fit 32 bits
    assert rows["full"] in seen[(254, 254), True] and rows["full_del"] in seen[(254, 254), True]
    assert rows["full"] not in seen[(255, 255), True] and rows["full_del"] not in seen[(0, 255), True]
    assert rows["full_del"] in seen[(255, 30), True]
    # a site's sums are the planes at the site
    got = bc.sites(0, 0, 0)
    assert len(got) == total.shape[1] and np.array_equal(got.counts, total.T)
    assert np.array_equal(got.bq_sums, bq.T) and np.array_equal(got.mq_sums, mq.T)


def test_sites_many_one_position_segments(bc):
    """5000 segments of one position each on a quality handle: more tiles than
    workgroups of one scan iteration (4096), the tiles around that edge sites
    at the thresholds, below the baseq one and below the mapq one."""
    rng = np.random.default_rng(37)
    S, edge = 5000, slice(4094, 4098)
    segs = [(int(rng.integers(0, N_REF)), i, i + 1) for i in rng.integers(0, 10 ** 6, size=S).tolist()]
    tids, starts, ends = arrays(segs)
    total = rng.integers(0, 25, size=(6, S)).astype(np.uint32)
    total[:, rng.random(S) < 0.2] = 0
    bq = (total * rng.integers(0, 256, size=(6, S))).astype(np.uint32)
    bq[DEL] = 0
    mq = (total * rng.integers(0, 256, size=(6, S))).astype(np.uint32)
    total[:, edge] = np.array([(30, 9, 0, 0, 2, 0)] * 4, np.uint32).T          # C: 9 of 39 beside the base allele A
    bq[:, edge] = np.array([(900, 180, 0, 0, 9, 0), (900, 181, 0, 0, 9, 0),    # C: 20 a, above, one below,
                            (900, 179, 0, 0, 9, 0), (900, 180, 0, 0, 9, 0)], np.uint32).T   # 20 a
    mq[:, edge] = np.array([(900, 270, 0, 0, 9, 0), (900, 2295, 0, 0, 9, 0),   # C: 30 a, 255 a, 30 a,
                            (900, 270, 0, 0, 9, 0), (900, 269, 0, 0, 9, 0)], np.uint32).T   # one below
    ref = rng.integers(0, 5, size=S).astype(np.uint8)
    ref[edge] = [0, 4, 0, 4]
    args = (10, 3, 100000)
    assert bc.begin(tids, starts, ends, quality=True) == S
    bc.set_counts(0, total, bq=bq, mq=mq)
    assert bc.timing()["tiles"] == S
    off = bc.seg_off
    with mb.BaseCounter(N_REF, 0) as plain:
        plain.begin(tids, starts, ends)
        plain.set_counts(0, total)
        for th, pattern in (((0, 0), [1, 1, 1, 1]), ((20, 30), [1, 1, 0, 0])):
            for r in (None, ref):
                got = bc.sites(*args, ref=r, min_alt_baseq=th[0], min_alt_mapq=th[1])
                first, pos, cnt, sb, sq = qm.sites_model(total, bq, mq, off, starts, *args, th[0], th[1], r)
                assert np.array_equal(got.first, first) and np.array_equal(got.pos, pos), (th, r is not None)
                assert np.array_equal(got.counts, cnt) and np.array_equal(got.bq_sums, sb)
                assert np.array_equal(got.mq_sums, sq)
                assert 0 < len(got) < S and np.diff(got.first)[edge].tolist() == pattern
                if th == (0, 0):
                    want = plain.sites(*args, ref=r)
                    assert np.array_equal(got.first, want.first) and np.array_equal(got.pos, want.pos)
                    assert np.array_equal(got.counts, want.counts)


# ------------------------------------------------- 7. state and argument errors

def raises(code, match, call):
    with pytest.raises(_lib.MetacovError, match=match) as e:
        call()
    assert e.value.code == code


def lib_sites_quality(bc, bq, mq):
    n = ctypes.c_int64()
    _lib.check(bc._lib.mc_bases_sites_quality(bc._h, 1, 1, 0, bq, mq, None, ctypes.byref(n)), bc._lib)
    return n.value


def test_track_argument_and_both_trackings(bc):
    lib = _lib.load()
    assert lib.mc_bases_track_quality(bc._h, 2) == _lib.MC_E_INVALID
    assert lib.mc_bases_track_quality(bc._h, -1) == _lib.MC_E_INVALID
    with pytest.raises(_lib.MetacovError) as e:
        bc.begin([0], [0], [10], strand=True, quality=True)
    assert e.value.code == _lib.MC_E_STATE
    assert "mc_bases_track_strand" in str(e.value) and "mc_bases_track_quality" in str(e.value)
    bc.begin([0], [0], [10], quality=True)                      # either alone is fine
    bc.begin([0], [0], [10], strand=True)


def test_reads_need_mapq_on_a_tracking_handle(bc):
    lib = _lib.load()
    b = bm.make_batch([(0, 3, "4M", "ACGT", 30)])
    ptrs = [_lib.ptr(x) for x in bm.batch_args(b)]
    flag, mapq = np.array([0x10], np.uint16), np.array([17], np.uint8)
    bc.begin([0], [0], [10], quality=True)
    with pytest.raises(ValueError, match="mapq"):
        bc.add_reads(*bm.batch_args(b))
    with pytest.raises(ValueError, match="mapq"):
        bc.add_reads(*bm.batch_args(b), flag=flag)
    assert lib.mc_bases_add_batch(bc._h, 1, *ptrs) == _lib.MC_E_STATE
    assert "mapq is needed (mc_bases_add_batch_mapq)" in lib.mc_last_error().decode()
    assert lib.mc_bases_add_batch_flags(bc._h, 1, *ptrs, _lib.ptr(flag)) == _lib.MC_E_STATE
    assert lib.mc_bases_add_batch_device(bc._h, 1, None, None, None, None, 0, None, None, None, 0, None, None,
                                         0) == _lib.MC_E_STATE
    assert "mc_bases_add_batch_device_mapq" in lib.mc_last_error().decode()
    assert lib.mc_bases_add_batch_mapq(bc._h, 1, *ptrs, None) == _lib.MC_E_INVALID      # the checks of add_batch
    assert "null read arrays" in lib.mc_last_error().decode()
    assert lib.mc_bases_add_batch_mapq(bc._h, -1, *ptrs, _lib.ptr(mapq)) == _lib.MC_E_INVALID
    bad = bm.make_batch([(0, 5, "4M", "ACGT", 30), (0, 3, "4M", "ACGT", 30)])
    raises(_lib.MC_E_INVALID, "read 1: reads are not sorted",
           lambda: bc.add_reads(*bm.batch_args(bad), mapq=[17, 17]))
    assert bc.counts().sum() == 0 and bc.quality()[1].sum() == 0
    bc.add_reads(*bm.batch_args(b), mapq=mapq)
    assert bc.quality()[0].sum() == 120 and bc.quality()[1].sum() == 68
    with pytest.raises(ValueError, match="inconsistent"):
        bc.add_reads(*bm.batch_args(b), mapq=[1, 2])


def test_new_calls_ignore_mapq_without_tracking(bc):
    b = bm.make_batch([(0, 3, "4M", "ACGT", 30)])
    bc.begin([0], [0], [10])
    bc.add_reads(*bm.batch_args(b), mapq=[200])
    bc.add_reads(*bm.batch_args(b))
    assert bc.counts()[:, 3:7].sum() == 8
    assert bc.sites().bq_sums is None


def test_fetch_needs_tracking(bc):
    lib = _lib.load()
    one = np.zeros((6, 1), np.uint32)
    bc.begin([0], [0], [10])
    for call in (lambda: bc.quality(), lambda: bc.set_counts(0, one, bq=one, mq=one),
                 lambda: lib_sites_quality(bc, 0, 0)):
        raises(_lib.MC_E_STATE, "does not track quality", call)
    p, q, st, nn = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
    r = ctypes.byref
    assert lib.mc_bases_quality_device(bc._h, r(p), r(q), r(st), r(nn)) == _lib.MC_E_STATE
    with pytest.raises(ValueError, match="min_alt_baseq"):
        bc.sites(min_alt_baseq=1)
    with pytest.raises(ValueError, match="min_alt_mapq"):
        bc.sites(min_alt_mapq=1)
    # with tracking the sums start from zero and are exposed on the device
    bc.begin([0], [0], [10], quality=True)
    assert bc.quality()[0].sum() == 0 and bc.quality()[1].sum() == 0
    assert lib.mc_bases_quality_device(bc._h, r(p), r(q), r(st), r(nn)) == _lib.MC_OK
    assert p.value and q.value and p.value != q.value and st.value >= 10 and nn.value == 10
    raises(_lib.MC_E_INVALID, "positions", lambda: bc.quality(5, 6))
    assert bc.quality(10, 0)[0].shape == (6, 0)


def test_set_quality_checks(bc):
    lib = _lib.load()
    bc.begin([0], [0], [10], quality=True)
    cnt = np.zeros((6, 2), np.uint32)
    cnt[T, 1], cnt[DEL, 0] = 3, 2
    ok_b, ok_m = np.zeros((6, 2), np.uint32), np.zeros((6, 2), np.uint32)
    ok_b[T, 1], ok_m[T, 1], ok_m[DEL, 0] = 765, 765, 510
    for ch, i, which, match in ((T, 1, 0, "baseq sum 766 exceeds 255 x count 3"),
                                (T, 1, 1, "mapq sum 766 exceeds 255 x count 3"),
                                (DEL, 0, 0, "baseq sum 1 "), (A, 0, 1, "mapq sum 1 exceeds 255 x count 0")):
        b, m = ok_b.copy(), ok_m.copy()
        (b, m)[which][ch, i] += 1
        raises(_lib.MC_E_INVALID, match, lambda: bc.set_counts(2, cnt, bq=b, mq=m))
        assert bc.counts().sum() == 0 and bc.quality()[0].sum() == 0 and bc.quality()[1].sum() == 0   # nothing written
    with pytest.raises(ValueError, match="together"):
        bc.set_counts(2, cnt, bq=ok_b)
    bc.add_reads(*bm.batch_args(bm.make_batch([(0, 0, "1M", "A", 30)])), mapq=[9])
    assert lib_sites_quality(bc, 0, 0) == 0
    bc.set_counts(2, cnt, bq=ok_b, mq=ok_m)                     # the sites are gone, as after mc_bases_set
    pos, c6 = np.zeros(1, np.int64), np.zeros((1, 6), np.uint32)
    assert lib.mc_bases_sites_get(bc._h, 0, 0, _lib.ptr(pos), _lib.ptr(c6)) == _lib.MC_E_STATE
    assert bc.quality()[0][T, 3] == 765 and bc.quality()[1][DEL, 2] == 510 and bc.counts()[T, 3] == 3
    bc.set_counts(2, np.zeros((6, 2), np.uint32))               # mc_bases_set leaves the sums alone
    assert bc.counts()[:, 2:4].sum() == 0 and bc.quality()[0][T, 3] == 765


def test_sites_quality_arguments_and_state(bc):
    lib = _lib.load()
    n = ctypes.c_int64()
    bc.begin([0], [0], [10], quality=True)
    bc.add_reads(*bm.batch_args(bm.make_batch([(0, 3, "4M", "ACGT", 30), (0, 3, "4M", "CCGT", 30)])), mapq=[9, 200])
    for bq, mq in ((-1, 0), (256, 0), (0, -1), (0, 256)):
        raises(_lib.MC_E_INVALID, "outside 0..255", lambda: lib_sites_quality(bc, bq, mq))
    assert lib_sites_quality(bc, 255, 255) == 0 and lib_sites_quality(bc, 30, 9) == 1
    b6, m6 = np.zeros((1, 6), np.uint32), np.zeros((1, 6), np.uint32)
    assert lib.mc_bases_sites_get_quality(bc._h, 0, 1, _lib.ptr(b6), _lib.ptr(m6)) == _lib.MC_OK
    assert b6.tolist() == [[30, 30, 0, 0, 0, 0]] and m6.tolist() == [[9, 200, 0, 0, 0, 0]]
    assert lib.mc_bases_sites_get_quality(bc._h, 1, 1, _lib.ptr(b6), _lib.ptr(m6)) == _lib.MC_E_INVALID
    # a plain sites call on the same handle leaves no sums of sites
    assert lib.mc_bases_sites(bc._h, 1, 1, 0, None, ctypes.byref(n)) == _lib.MC_OK and n.value == 1
    assert lib.mc_bases_sites_get_quality(bc._h, 0, 1, _lib.ptr(b6), _lib.ptr(m6)) == _lib.MC_E_STATE
    assert "mc_bases_sites_quality" in lib.mc_last_error().decode()
    # nor does a strand sites call
    bc.begin([0], [0], [10], strand=True)
    bc.add_reads(*bm.batch_args(bm.make_batch([(0, 3, "4M", "ACGT", 30), (0, 3, "4M", "CCGT", 30)])), flag=[0, 16])
    assert len(bc.sites()) == 1
    assert lib.mc_bases_sites_get_quality(bc._h, 0, 1, _lib.ptr(b6), _lib.ptr(m6)) == _lib.MC_E_STATE


def test_counts_results_unchanged_by_tracking(bc, random_reads):
    """mc_bases_get, _sites, _consensus and _insertions with tracking on as off."""
    b, mapq, segs = random_reads
    tids, starts, ends = arrays(segs)
    out = []
    for quality in (False, True):
        bc.begin(tids, starts, ends, min_baseq=10, insertions=True, quality=quality)
        bc.add_reads(*bm.batch_args(b), mapq=mapq)
        s, ins = bc.sites(3, 2, 100000), bc.insertions(1, 1, 0)
        cons = bc.consensus(2, 1, 500000, iupac=True)
        out.append([bc.counts(), s.first, s.pos, s.counts, ins.index, ins.length, ins.code, ins.count, cons.first,
                    cons.summary] + [cons.compact(k) for k in range(len(segs))])
    assert len(out[0][2]) > 0 and len(out[0][4]) > 0
    assert all(np.array_equal(x, y) for x, y in zip(*out))


# ------------------------------------------------------------------ 8. GPU decode

@pytest.fixture(scope="module")
def host_planes(lib_built, golden_dir):
    """Counts and sums of each golden BAM through the host source, computed once."""
    out = {}
    for name in GOLDENS:
        path = os.path.join(golden_dir, name)
        lengths = bm.kept_reads(path)[1]
        with mb.BaseCounter(len(lengths), 0) as h:
            h.begin(np.arange(len(lengths)), np.zeros(len(lengths), np.int64), lengths, min_baseq=10, quality=True)
            h.add_bam(path)
            out[name] = (lengths, h.counts()) + h.quality() + (qm.kept_mapq(path),)
    return out


@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("window", [0, 1 << 20])
def test_gpu_decode(host_planes, golden_dir, name, window):
    path = os.path.join(golden_dir, name)
    lengths, total, bq, mq, mapq = host_planes[name]
    with mb.GpuBaseSource(path, 0, window_bytes=window) as src, mb.BaseCounter(len(lengths), 0) as h:
        got = src.copy_mapq()
        assert got.dtype == np.uint8 and np.array_equal(got, mapq)
        assert set(src.copy()) == {"tid", "pos", "cig_off", "cigar", "l_seq", "seq_off", "seq", "qual_off", "qual"}
        for max_reads in (1 << 20, 97):                          # sub-ranges cut inside piles
            h.begin(np.arange(len(lengths)), np.zeros(len(lengths), np.int64), lengths, min_baseq=10, quality=True)
            h.add_device(src, max_reads=max_reads)
            got_bq, got_mq = h.quality()
            assert np.array_equal(h.counts(), total), max_reads
            assert np.array_equal(got_bq, bq) and np.array_equal(got_mq, mq), max_reads
    with mb.GpuBaseSource(path, 0, min_mapq=30, window_bytes=window) as src:
        assert np.array_equal(src.copy_mapq(), qm.kept_mapq(path, min_mapq=30))
    if name == "bbmap.sorted.bam":
        assert bq.sum() > 0 and mq.sum() > 0 and len(set(mapq.tolist())) >= 2
        b = bm.kept_reads(path)[2]
        _, want_total, want_bq, want_mq = qm.counts_model(b, mapq, np.arange(len(lengths)),
                                                          np.zeros(len(lengths), np.int64), lengths, 10)
        same(total, want_total, "total")
        same(bq, want_bq, "bq")
        same(mq, want_mq, "mq")


# ------------------------------------------------------------------------ 9. CLI

def test_cli_quality(lib_built, golden_dir, tmp_path, host_planes):
    from metacov_amd.cli import main
    path = os.path.join(golden_dir, "bbmap.sorted.bam")
    fa = os.path.join(golden_dir, "reference_1K.fa.gz")
    names = bm.kept_reads(path)[0]

    def cli(tag, *args):
        o = tmp_path / (tag + ".tsv")
        res = CliRunner().invoke(main, ["bases", "-b", path, "-o", str(o)] + list(args))
        assert res.exit_code == 0, res.output
        return o.read_text()

    for k, args in enumerate((["--all", "--min-baseq", "10"], ["-f", fa, "--min-depth", "4", "--min-count", "2"])):
        host = cli("h%d" % k, "--quality", "--decode", "host", *args)
        assert host == cli("g%d" % k, "--quality", "--decode", "gpu", *args) and host.count("\n") > 1
        plain = cli("p%d" % k, *args)
        assert "\n".join("\t".join(ln.split("\t")[:10]) for ln in host.split("\n")) == plain
        assert all(len(ln.split("\t")) == 21 for ln in host.split("\n")[:-1])
    # --all: the eleven columns are the host path's planes
    lengths, total, bq, mq, _ = host_planes["bbmap.sorted.bam"]
    off = bm.seg_offsets(np.zeros(len(lengths), np.int64), lengths)
    rows = [(t, p, total[:, off[t] + p], bq[:, off[t] + p], mq[:, off[t] + p])
            for t in range(len(lengths)) for p in range(lengths[t])]
    assert cli("all", "--quality", "--all", "--min-baseq", "10") == qm.table(dict(enumerate(names)), rows)
    # both thresholds: the model's sites.  The reads carry next to no variants, so the reference is changed
    # at every third position: there the reads' base is the alternative allele, and it is a site where its
    # mean qualities reach the thresholds
    swap = str.maketrans("ACGT", "CATG")
    mut = {n: "".join(ch.translate(swap) if i % 3 == 0 else ch for i, ch in enumerate(v.upper()))
           for n, v in bm.read_fasta(fa).items()}
    mfa = tmp_path / "changed.fa"
    mfa.write_text("".join(">%s\n%s\n" % kv for kv in mut.items()))
    ref = mb.ref_codes(np.concatenate([np.frombuffer(mut[n].encode(), np.uint8) for n in names]))
    assert len(ref) == total.shape[1]
    starts = np.zeros(len(lengths), np.int64)
    first, pos, cnt, sb, sq = qm.sites_model(total, bq, mq, off, starts, 1, 2, 20000, CLI_BASEQ, CLI_MAPQ, ref)
    rows = [(t, int(pos[i]), cnt[i], sb[i], sq[i]) for t in range(len(lengths)) for i in range(first[t], first[t + 1])]
    plain_n = len(bm.sites_model(total, off, starts, 1, 2, 20000, ref)[1])
    assert 0 < len(rows) < plain_n
    args = ["--quality", "--min-alt-baseq", str(CLI_BASEQ), "--min-alt-mapq", str(CLI_MAPQ), "--min-baseq", "10",
            "--min-count", "2", "--min-frac", "0.02", "-f", str(mfa)]
    got = cli("q", *args)
    assert got == qm.table(dict(enumerate(names)), rows, mut)
    assert got == cli("qg", "--decode", "gpu", *args)
    assert cli("q0", "--quality", *args[5:]).count("\n") == plain_n + 1      # thresholds 0: the plain predicate's sites

