"""Strand-resolved base counts on the GPU (csrc/bases.hip, the strand
instantiation of the pileup kernel and the strand sites kernels) against
tests/strand_model.py: exact equality of both plane sets, the sites and the
CLI's bytes.  Shapes are a few tiles at most; P comes from the library."""
import ctypes
import os

import numpy as np
import pytest
from click.testing import CliRunner

from metacov_amd import _lib
from metacov_amd import bases as mb
from tests import bases_model as bm
from tests import strand_model as sm
from tests.bases_model import A, C, G, T, N, DEL

pytestmark = pytest.mark.gpu

N_REF = 4
GOLDENS = ["bbmap.sorted.bam", "synth_edge.bam", "synth_exp.bam", "synth_exp_noseq.bam", "synth_longcigar.bam",
           "synth_multi.bam"]


@pytest.fixture(scope="module")
def bc(lib_built):
    h = mb.BaseCounter(N_REF, 0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def P(lib_built):
    return mb.dims()


def arrays(segs):
    return tuple(np.array(x, np.int64) for x in zip(*segs))


def run(bc, batches, flags, segs, min_baseq=0, strand=True):
    """(total, rev) of a strand-tracking counter, or (total, None)."""
    tids, starts, ends = arrays(segs)
    n = bc.begin(tids, starts, ends, min_baseq=min_baseq, strand=strand)
    for b, f in zip(batches, flags):
        bc.add_reads(*bm.batch_args(b), flag=f if strand else None)
    total = bc.counts()
    assert total.dtype == np.uint32 and total.shape == (6, n)
    if not strand:
        return total, None
    rev = bc.counts_reverse()
    assert rev.dtype == np.uint32 and rev.shape == (6, n)
    return total, rev


def same(got, want, what):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: first difference at (channel, index) %s: got %d, want %d" % (
        what, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def check(bc, batches, flags, segs, min_baseq=0, loop=False):
    """Both plane sets against the model, the totals against an unstranded
    counter fed the same reads."""
    if isinstance(batches, dict):
        batches, flags = [batches], [flags]
    tids, starts, ends = arrays(segs)
    total, rev = run(bc, batches, flags, segs, min_baseq)
    _, want_total, want_rev = sm.counts_model(batches, flags, tids, starts, ends, min_baseq, loop=loop)
    same(total, want_total, "total")
    same(rev, want_rev, "reverse")
    assert (rev <= total).all()
    plain, _ = run(bc, batches, flags, segs, min_baseq, strand=False)
    assert np.array_equal(plain, total)
    return total, rev


def random_flags(rng, n):
    """0 or 0x10, OR-ed with random other bits that must not matter."""
    f = rng.integers(0, 2, size=n) * 0x10
    for bit in (0x1, 0x40, 0x80, 0x800):
        f |= rng.integers(0, 2, size=n) * bit
    return f.astype(np.uint16)


# ------------------------------------------------------------- 1. random reads

CIGARS = ["40M", "12M3I20M", "15M4D15M", "10M30N12M", "5S25M", "25M6S", "3H20M2H", "8=2X8=",
          "2H3S5M2I4M3D6M7N2=1X1P2M4S", "1M", "60M", "7M1D7M1I7M"]


@pytest.fixture(scope="module")
def random_reads(P):
    """About 400 reads over 3 contigs of more than one tile, with their flags."""
    rng = np.random.default_rng(21)
    lengths = [2 * P + 77, P - 3, 300]
    reads = []
    for _ in range(400):
        t = int(rng.choice(3, p=[.6, .3, .1]))
        c = str(rng.choice(CIGARS))
        k = bm.query_length(bm.cigar_words(c))
        q = None if rng.random() < .15 else [int(x) for x in rng.integers(0, 41, size=k)]
        reads.append((t, int(rng.integers(0, lengths[t] - 20)), c,
                      "".join(rng.choice(list("ACGTN"), size=k, p=[.24, .24, .24, .24, .04])), q))
    reads.sort(key=lambda r: (r[0], r[1]))
    b = bm.make_batch(reads)
    assert set("".join(CIGARS)) >= set("MIDNSH=X")
    return b, random_flags(rng, len(reads)), [(t, 0, L) for t, L in enumerate(lengths)]


@pytest.mark.parametrize("min_baseq", [0, 20])
def test_random_reads(bc, random_reads, min_baseq):
    b, flags, segs = random_reads
    absent = sum(int(b["qual"][int(b["qual_off"][i])]) == 0xFF for i in range(bm.n_reads(b)))
    assert 20 < absent < 120 and 100 < int(sm.is_reverse(flags).sum()) < 300
    total, rev = check(bc, b, flags, segs, min_baseq)
    assert 0 < rev.sum() < total.sum() and rev[DEL].sum() > 0 and (total - rev)[DEL].sum() > 0


# ---------------------------------------------------- 2. tile and segment edges

def test_tile_and_segment_edges(bc, P):
    rng = np.random.default_rng(22)

    def rd(t, pos, cigar):
        k = bm.query_length(bm.cigar_words(cigar))
        return (t, pos, cigar, "".join(rng.choice(list("ACGT"), size=k)), 30)

    reads, flags = [], []
    for edge in (P, 2 * P):
        for f in (0, 0x10):
            for r in (rd(0, edge - 30, "60M"), rd(0, edge - 1, "1M"), rd(0, edge, "1M"), rd(0, edge - 1, "2M"),
                      rd(0, edge - 20, "15M10D15M"), rd(0, edge - 10, "10M5I10M"), rd(0, edge - 40, "40M")):
                reads.append(r)
                flags.append(f)
    # reverse reads whose only overlap with a tile is a deletion: three positions of the second tile, and
    # the whole of it
    for r in (rd(0, P - 10, "10M3D"), rd(0, P - 5, "5M%dD5M" % P)):
        reads.append(r)
        flags.append(0x10 | 0x80)
    reads += [rd(1, 0, "30M"), rd(1, 4, "10M2D10M"), rd(1, P, "8M")]
    flags += [0x10, 0, 0x10]
    order = sorted(range(len(reads)), key=lambda i: (reads[i][0], reads[i][1]))
    b = bm.make_batch([reads[i] for i in order])
    flags = np.array([flags[i] for i in order], np.uint16)
    # segments at plane offsets 1, 2 and 3 past a multiple of four (lead != 0), an overlapping, a duplicated
    # and an empty one
    segs = [(0, 0, 2 * P + 101), (0, 5, P + 6), (1, 9, 9), (0, 0, 2 * P + 101), (1, 3, P + 8), (0, P - 1, P + 1)]
    off = bm.seg_offsets([s[1] for s in segs], [s[2] for s in segs])
    assert P % 4 == 0 and [int(o) & 3 for o in off[1:5]] == [1, 2, 2, 3] and off[2] == off[3]
    total, rev = check(bc, b, flags, segs)
    second = slice(P, 2 * P)                                    # the first segment's second tile
    assert rev[DEL, second].min() >= 1 and total[DEL, second].max() >= 2
    assert np.array_equal(total[:, :2 * P + 101], total[:, int(off[3]):int(off[4])])
    assert np.array_equal(rev[:, :2 * P + 101], rev[:, int(off[3]):int(off[4])])


# -------------------------------------------------------- 3. batch independence

def test_batch_independence(bc, random_reads):
    b, flags, segs = random_reads
    n = bm.n_reads(b)
    want = None
    for parts in (1, 2, 7):
        cuts = [n * k // parts for k in range(parts + 1)]
        batches = [bm.slice_batch(b, x, y) for x, y in zip(cuts, cuts[1:])]
        got = run(bc, batches, [flags[x:y] for x, y in zip(cuts, cuts[1:])], segs, 20)
        if want is None:
            want = got
            assert want[1].sum() > 0
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), parts


# ----------------------------------------------------- 4. counter-width boundary

def one_base_reads(tid, pos, n):
    """n reads `1M` with base A at (tid, pos), as a batch."""
    ar = np.arange(n + 1, dtype=np.int64)
    return {"tid": np.full(n, tid, np.int32), "pos": np.full(n, pos, np.int32), "l_seq": np.ones(n, np.int32),
            "cig_off": ar, "cigar": np.full(n, (1 << 4) | 0, np.uint32), "seq_off": ar,
            "seq": np.full(n, 0x10, np.uint8), "qual_off": ar, "qual": np.full(n, 30, np.uint8)}


def test_counter_width_boundary(bc):
    """One-base reads piled on one position: 65535 reads are the most a tile
    counts in 16-bit halves; 65536 forward reads would carry out of the low
    half into the reverse one."""
    rng = np.random.default_rng(24)
    piles = [(40000, 25535), (65536, 0), (3, 70000)]
    batches, flags = [], []
    for t, (fwd, rv) in enumerate(piles):
        f = np.concatenate([np.zeros(fwd, np.uint16), np.full(rv, 0x10, np.uint16)])
        rng.shuffle(f)
        batches.append(one_base_reads(t, 5, fwd + rv))
        flags.append(f)
    assert [bm.n_reads(b) for b in batches] == [65535, 65536, 70003]
    segs = [(0, 0, 8), (1, 0, 8), (2, 0, 8)]
    total, rev = run(bc, batches, flags, segs)
    want_total, want_rev = np.zeros((6, 24), np.uint32), np.zeros((6, 24), np.uint32)
    for t, (fwd, rv) in enumerate(piles):
        want_total[A, 8 * t + 5] = fwd + rv
        want_rev[A, 8 * t + 5] = rv
    same(total, want_total, "total")
    same(rev, want_rev, "reverse")
    plain, _ = run(bc, batches, flags, segs, strand=False)
    assert np.array_equal(plain, total)


# ------------------------------------------------------------------ 5. int32 edge

def test_int32_edge(bc, P):
    reads, segs, _, k = bm.int32_edge_case(P)
    b = bm.make_batch(reads)
    n = bm.n_reads(b)
    flags = random_flags(np.random.default_rng(25), n)
    assert int(b["pos"].max()) == (1 << 31) - 1 and 0 < k < n
    batches = [bm.slice_batch(b, 0, k), bm.slice_batch(b, k, n)]
    total, rev = check(bc, batches, [flags[:k], flags[k:]], segs, loop=True)
    assert 0 < rev.sum() < total.sum()


# ------------------------------------------------------- 6. sites on crafted planes

def crafted_planes(P, segs):
    """Totals, reverse counts and a reference plane over the segments: random
    background without alternative alleles, then the rows of interest."""
    rng = np.random.default_rng(26)
    off = bm.seg_offsets([s[1] for s in segs], [s[2] for s in segs])
    n = int(off[-1])
    total, rev = np.zeros((6, n), np.uint32), np.zeros((6, n), np.uint32)
    total[A] = rng.integers(0, 40, size=n)                       # one allele only: no site
    rev[A] = rng.integers(0, 41, size=n) * total[A] // 40
    total[N] = rng.integers(0, 3, size=n)
    rev[N] = total[N] // 2
    ref = np.full(n, 4, np.uint8)

    def put(i, t, r, rf=4):
        total[:, i], rev[:, i], ref[i] = t, r, rf

    rows = {}
    #                       A   C  G  T  N DEL
    rows["one_strand"] = (10, [30, 8, 0, 0, 0, 0], [15, 0, 0, 0, 0, 0])        # C on the forward strand only
    rows["weaker_ok"] = (11, [30, 8, 0, 4, 1, 0], [15, 8, 0, 2, 0, 0])         # C one-stranded, T 2 + 2
    rows["weaker_few"] = (12, [30, 8, 0, 2, 0, 0], [15, 8, 0, 1, 0, 0])        # T fails min_count 3
    rows["ref_minority"] = (13, [30, 6, 0, 0, 0, 0], [12, 6, 0, 0, 0, 0], 1)   # ref C: A is the alternative
    rows["ref_unknown"] = (14, [6, 30, 0, 0, 0, 0], [3, 13, 0, 0, 0, 0], 4)    # ref = 4: base C, alt A 3 + 3
    rows["del_alt"] = (15, [30, 0, 0, 0, 0, 9], [15, 0, 0, 0, 0, 4])           # DEL 5 + 4
    rows["del_one_strand"] = (16, [30, 0, 0, 0, 0, 9], [15, 0, 0, 0, 0, 9])
    for v in rows.values():
        put(*v)
    both = ([20, 0, 6, 0, 0, 0], [10, 0, 3, 0, 0, 0])
    places = [P - 1, P, 2 * P - 1, 2 * P, int(off[1]), int(off[1]) + P - 2, int(off[1]) + P - 1, int(off[2]) - 1,
              int(off[2]), int(off[2]) + 17, n - 1]
    assert len(set(places)) == len(places) and min(places) > 100 and max(places) == n - 1
    for i in places:                                            # tile edges, segment ends, unaligned segments
        put(i, *both)
    assert (rev <= total).all()
    return off, total, rev, ref, rows, places


def test_sites_on_crafted_planes(bc, P):
    segs = [(0, 0, 2 * P + 1), (1, 100, 100 + P + 2), (2, 7, 7 + 50)]        # the later ones start at offsets 1 and 3
    tids, starts, ends = arrays(segs)
    off, total, rev, ref, rows, places = crafted_planes(P, segs)
    assert [int(o) & 3 for o in off[1:3]] == [1, 3]
    bc.begin(tids, starts, ends, strand=True)
    bc.set_counts(0, total, rev=rev)
    assert np.array_equal(bc.counts(), total) and np.array_equal(bc.counts_reverse(), rev)
    with mb.BaseCounter(N_REF, 0) as plain:
        plain.begin(tids, starts, ends)
        plain.set_counts(0, total)
        for r in (None, ref):
            want = plain.sites(4, 3, 50000, ref=r)
            got = bc.sites(4, 3, 50000, ref=r, min_alt_strand=0)
            assert want.rev_counts is None and len(want) > len(places)
            assert np.array_equal(got.first, want.first) and np.array_equal(got.pos, want.pos)
            assert np.array_equal(got.counts, want.counts)
            assert np.array_equal(got.rev_counts, rev[:, off[0] + _plane_index(got, off, starts)].T)
    seen = {}
    for K in (1, 2, 3):
        for r in (None, ref):
            got = bc.sites(4, 3, 50000, ref=r, min_alt_strand=K)
            first, pos, cnt, rc = sm.sites_model(total, rev, off, starts, 4, 3, 50000, K, r)
            assert np.array_equal(got.first, first) and np.array_equal(got.pos, pos), (K, r is not None)
            assert np.array_equal(got.counts, cnt) and np.array_equal(got.rev_counts, rc)
            assert got.rev_counts.dtype == np.uint32 and got.rev_counts.shape == (len(got), 6)
            seen[K, r is not None] = set(_plane_index(got, off, starts).tolist())
    at = {k: v[0] for k, v in rows.items()}
    s = seen[2, True]
    assert at["one_strand"] not in s and at["weaker_ok"] in s and at["weaker_few"] not in s
    assert at["ref_minority"] in s and at["ref_unknown"] in s and at["del_alt"] in s and at["del_one_strand"] not in s
    assert at["ref_minority"] not in seen[2, False]             # without ref A is the base allele there
    assert set(places) <= seen[3, True] and at["ref_unknown"] in seen[3, True] and at["del_alt"] in seen[3, True]
    assert at["weaker_ok"] not in seen[3, True]
    # a site's reverse counts are the reverse planes at the site
    got = bc.sites(0, 0, 0, min_alt_strand=0)
    assert len(got) == total.shape[1] and np.array_equal(got.rev_counts, rev.T) and np.array_equal(got.counts, total.T)


def test_sites_many_one_position_segments(bc):
    """5000 segments of one position each on a strand handle: more tiles than
    one scan iteration (4096), the tiles around that edge sites on both
    strands, on one, and too weak on one."""
    rng = np.random.default_rng(22)
    S, edge = 5000, slice(4094, 4098)
    segs = [(int(rng.integers(0, N_REF)), i, i + 1) for i in rng.integers(0, 10 ** 6, size=S).tolist()]
    tids, starts, ends = arrays(segs)
    total = rng.integers(0, 25, size=(6, S)).astype(np.uint32)
    total[:, rng.random(S) < 0.2] = 0
    rev = (total * rng.random((6, S))).astype(np.uint32)
    total[:, edge] = np.array([(30, 9, 0, 0, 2, 0)] * 4, np.uint32).T          # C: 9 of 39 beside the base allele A
    rev[:, edge] = np.array([(15, 4, 0, 0, 1, 0), (15, 2, 0, 0, 1, 0),         # C: 5 + 4, 7 + 2,
                             (15, 9, 0, 0, 1, 0), (15, 1, 0, 0, 1, 0)], np.uint32).T   # 0 + 9 and 8 + 1
    assert (rev <= total).all()
    ref = rng.integers(0, 5, size=S).astype(np.uint8)
    ref[edge] = [0, 4, 0, 4]
    args = (10, 3, 100000)
    assert bc.begin(tids, starts, ends, strand=True) == S
    bc.set_counts(0, total, rev=rev)
    assert bc.timing()["tiles"] == S
    off = bc.seg_off
    with mb.BaseCounter(N_REF, 0) as plain:
        plain.begin(tids, starts, ends)
        plain.set_counts(0, total)
        for K, pattern in ((0, [1, 1, 1, 1]), (2, [1, 1, 0, 0])):
            for r in (None, ref):
                got = bc.sites(*args, ref=r, min_alt_strand=K)
                first, pos, cnt, rc = sm.sites_model(total, rev, off, starts, *args, K, r)
                assert np.array_equal(got.first, first) and np.array_equal(got.pos, pos), (K, r is not None)
                assert np.array_equal(got.counts, cnt) and np.array_equal(got.rev_counts, rc)
                assert 0 < len(got) < S and np.diff(got.first)[edge].tolist() == pattern
                if K == 0:
                    want = plain.sites(*args, ref=r)
                    assert np.array_equal(got.first, want.first) and np.array_equal(got.pos, want.pos)
                    assert np.array_equal(got.counts, want.counts)


def _plane_index(sites, off, starts):
    """Plane indices of the sites."""
    out = np.zeros(len(sites), np.int64)
    for s in range(len(starts)):
        a, b = int(sites.first[s]), int(sites.first[s + 1])
        out[a:b] = sites.pos[a:b] - int(starts[s]) + int(off[s])
    return out


# ------------------------------------------------- 7. state and argument errors

def test_state_and_argument_errors(bc):
    lib = _lib.load()
    b = bm.make_batch([(0, 3, "4M", "ACGT", 30)])
    one = np.zeros((6, 1), np.uint32)
    n = ctypes.c_int64()
    bc.begin([0], [0], [10], strand=True)
    with pytest.raises(ValueError, match="flags"):
        bc.add_reads(*bm.batch_args(b))
    assert lib.mc_bases_add_batch(bc._h, 1, *[_lib.ptr(x) for x in bm.batch_args(b)]) == _lib.MC_E_STATE
    assert "flags are needed" in lib.mc_last_error().decode()
    assert lib.mc_bases_add_batch_device(bc._h, 1, None, None, None, None, 0, None, None, None, 0, None, None,
                                         0) == _lib.MC_E_STATE
    assert bc.counts().sum() == 0
    with pytest.raises(_lib.MetacovError, match="min_alt_strand") as e:
        bc.sites(min_alt_strand=-1)
    assert e.value.code == _lib.MC_E_INVALID
    hi = one.copy()
    hi[T, 0] = 4
    lo = one.copy()
    lo[T, 0] = 3
    with pytest.raises(_lib.MetacovError, match="reverse count 4 exceeds total 3") as e:
        bc.set_counts(2, lo, rev=hi)
    assert e.value.code == _lib.MC_E_INVALID
    assert bc.counts().sum() == 0 and bc.counts_reverse().sum() == 0      # nothing was written
    bc.add_reads(*bm.batch_args(b), flag=[0x10])
    bc.sites()
    bc.set_counts(2, hi, rev=lo)                                          # the sites are gone, as after mc_bases_set
    pos, cnt = np.zeros(1, np.int64), np.zeros((1, 6), np.uint32)
    assert lib.mc_bases_sites_get(bc._h, 0, 0, _lib.ptr(pos), _lib.ptr(cnt)) == _lib.MC_E_STATE
    assert bc.counts_reverse()[T, 2] == 3 and bc.counts()[T, 2] == 4
    # a plain sites call leaves no reverse counts of sites
    assert lib.mc_bases_sites(bc._h, 1, 0, 0, None, ctypes.byref(n)) == _lib.MC_OK and n.value == 5
    assert lib.mc_bases_sites_get_reverse(bc._h, 0, 1, _lib.ptr(cnt)) == _lib.MC_E_STATE
    assert lib.mc_bases_track_strand(bc._h, 2) == _lib.MC_E_INVALID
    # a second begin without tracking: no reverse planes, the flags are ignored
    bc.begin([0], [0], [10])
    for call in (lambda: bc.counts_reverse(), lambda: bc.set_counts(0, one, rev=one),
                 lambda: lib_sites_strand(bc, 0)):
        with pytest.raises(_lib.MetacovError) as e:
            call()
        assert e.value.code == _lib.MC_E_STATE and "does not track strand" in str(e.value)
    d, st, nn = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
    assert lib.mc_bases_reverse_device(bc._h, ctypes.byref(d), ctypes.byref(st), ctypes.byref(nn)) == _lib.MC_E_STATE
    with pytest.raises(ValueError, match="min_alt_strand"):
        bc.sites(min_alt_strand=1)
    assert bc.sites().rev_counts is None
    bc.add_reads(*bm.batch_args(b), flag=[0x10])
    bc.add_reads(*bm.batch_args(b))
    assert bc.counts()[:, 3:7].sum() == 8
    # with tracking again the reverse planes start from zero and are exposed on the device
    bc.begin([0], [0], [10], strand=True)
    assert bc.counts_reverse().sum() == 0
    assert lib.mc_bases_reverse_device(bc._h, ctypes.byref(d), ctypes.byref(st), ctypes.byref(nn)) == _lib.MC_OK
    assert d.value and st.value >= 10 and nn.value == 10


def lib_sites_strand(bc, k):
    n = ctypes.c_int64()
    _lib.check(bc._lib.mc_bases_sites_strand(bc._h, 1, 1, 0, k, None, ctypes.byref(n)), bc._lib)


# ------------------------------------------------------------------ 8. GPU decode

@pytest.fixture(scope="module")
def host_planes(lib_built, golden_dir):
    """Both plane sets of each golden BAM through the host source, computed once."""
    out = {}
    for name in GOLDENS:
        path = os.path.join(golden_dir, name)
        lengths = bm.kept_reads(path)[1]
        with mb.BaseCounter(len(lengths), 0) as h:
            h.begin(np.arange(len(lengths)), np.zeros(len(lengths), np.int64), lengths, min_baseq=10, strand=True)
            h.add_bam(path)
            out[name] = (lengths, h.counts(), h.counts_reverse(), sm.kept_flags(path))
    return out


@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("window", [0, 1 << 20])
def test_gpu_decode(host_planes, golden_dir, name, window):
    path = os.path.join(golden_dir, name)
    lengths, total, rev, flags = host_planes[name]
    with mb.GpuBaseSource(path, 0, window_bytes=window) as src, mb.BaseCounter(len(lengths), 0) as h:
        got = src.copy_flags()
        assert got.dtype == np.uint16 and np.array_equal(got, flags)
        assert set(src.copy()) == {"tid", "pos", "cig_off", "cigar", "l_seq", "seq_off", "seq", "qual_off", "qual"}
        for max_reads in (1 << 20, 97):                          # sub-ranges cut inside piles
            h.begin(np.arange(len(lengths)), np.zeros(len(lengths), np.int64), lengths, min_baseq=10, strand=True)
            h.add_device(src, max_reads=max_reads)
            assert np.array_equal(h.counts(), total) and np.array_equal(h.counts_reverse(), rev), max_reads
    if name == "bbmap.sorted.bam":
        assert rev.sum() > 0 and (total - rev).sum() > 0 and 0 < int(sm.is_reverse(flags).sum()) < len(flags)
        b = bm.kept_reads(path)[2]
        _, want_total, want_rev = sm.counts_model(b, flags, np.arange(len(lengths)), np.zeros(len(lengths), np.int64),
                                                  lengths, 10)
        same(total, want_total, "total")
        same(rev, want_rev, "reverse")


# ------------------------------------------------------------------------ 9. CLI

def test_cli_strand(lib_built, golden_dir, tmp_path, host_planes):
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
        host = cli("h%d" % k, "--strand", "--decode", "host", *args)
        assert host == cli("g%d" % k, "--strand", "--decode", "gpu", *args) and host.count("\n") > 1
        plain = cli("p%d" % k, *args)
        assert "\n".join("\t".join(ln.split("\t")[:10]) for ln in host.split("\n")) == plain
        assert all(len(ln.split("\t")) == 22 for ln in host.split("\n")[:-1])
    # --all: the twelve columns are the host path's planes
    lengths, total, rev, _ = host_planes["bbmap.sorted.bam"]
    off = bm.seg_offsets(np.zeros(len(lengths), np.int64), lengths)
    rows = [(t, p, total[:, off[t] + p], rev[:, off[t] + p]) for t in range(len(lengths)) for p in range(lengths[t])]
    assert cli("all", "--strand", "--all", "--min-baseq", "10") == sm.table(dict(enumerate(names)), rows)
    # --min-alt-strand 2: the model's sites.  The reads carry next to no variants, so the reference is
    # changed at every third position: there the reads' base is the alternative allele, and it is a site
    # where both strands see it twice (not at the contig ends, which one strand alone covers)
    swap = str.maketrans("ACGT", "CATG")
    mut = {n: "".join(ch.translate(swap) if i % 3 == 0 else ch for i, ch in enumerate(v.upper()))
           for n, v in bm.read_fasta(fa).items()}
    mfa = tmp_path / "changed.fa"
    mfa.write_text("".join(">%s\n%s\n" % kv for kv in mut.items()))
    ref = mb.ref_codes(np.concatenate([np.frombuffer(mut[n].encode(), np.uint8) for n in names]))
    assert len(ref) == total.shape[1]
    starts = np.zeros(len(lengths), np.int64)
    first, pos, cnt, rc = sm.sites_model(total, rev, off, starts, 1, 2, 20000, 2, ref)
    rows = [(t, int(pos[i]), cnt[i], rc[i]) for t in range(len(lengths)) for i in range(first[t], first[t + 1])]
    plain_n = len(bm.sites_model(total, off, starts, 1, 2, 20000, ref)[1])
    assert 100 < len(rows) < plain_n
    args = ["--strand", "--min-alt-strand", "2", "--min-baseq", "10", "--min-count", "2", "--min-frac", "0.02",
            "-f", str(mfa)]
    got = cli("k2", *args)
    assert got == sm.table(dict(enumerate(names)), rows, mut)
    assert got == cli("k2g", "--decode", "gpu", *args)
    assert cli("k0", "--strand", *args[3:]).count("\n") == plain_n + 1       # K = 0: the plain predicate's sites
