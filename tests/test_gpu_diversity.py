"""Windowed diversity on the GPU (csrc/bases_div.h) against the model in
tests/diversity_model.py: exact equality of win_first and of every row.
Planes are set through set_counts (mc_bases_set) except in the end-to-end
tests; shapes are a few tiles at most; P (tile positions) comes from the
library."""
import ctypes
import io
import re

import numpy as np
import pytest
from click.testing import CliRunner

from metacov_amd import _lib
from metacov_amd import bases as mb
from tests import bases_model as bm
from tests import diversity_model as dm
from tests.test_gpu_consensus import golden, random_cigar, region_planes

pytestmark = pytest.mark.gpu

N_REF = 4


@pytest.fixture(scope="module")
def bc(lib_built):
    h = mb.BaseCounter(N_REF, 0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def P(lib_built):
    return mb.dims()


def begin(bc, segs, planes=None):
    tids, starts, ends = (np.array(x, np.int64) for x in zip(*segs)) if segs else (np.zeros(0, np.int64),) * 3
    n = bc.begin(tids, starts, ends)
    if planes is not None:
        assert planes.shape == (6, n)
        bc.set_counts(0, planes)
    return bc.seg_off


def random_planes(rng, n, hi=5, p_mono=0.5, p_empty=0.1, dels=True):
    """Small counts with ties; half the positions monomorphic, some empty."""
    planes = rng.integers(0, hi, size=(6, n)).astype(np.uint32)
    if not dels:
        planes[bm.DEL] = 0
    mono = rng.random(n) < p_mono
    keep = rng.integers(0, 4, size=n)
    for c in range(4):
        planes[c, mono & (keep != c)] = 0
    planes[:, rng.random(n) < p_empty] = 0
    return planes


def check(bc, planes, seg_off, window=0, **kw):
    got = bc.diversity(window, **kw)
    first, rows = dm.diversity_model(planes, seg_off, window, **kw)
    assert got.rows.dtype == np.int64 and got.rows.shape == rows.shape
    assert np.array_equal(got.win_first, first)
    bad = np.argwhere(got.rows != rows)
    assert len(bad) == 0, "window %d: rows differ first at (row, column) %s: got %s, want %s" % (
        window, bad[0], got.rows[bad[0][0]], rows[bad[0][0]])
    assert got.rows[:, dm.POSITIONS].sum() == planes.shape[1]
    return got


# --------------------------------------------------------------------- rule

def test_rule_by_hand(bc):
    #        A  C  G  T   r    covered snv q                 compared con pop   (min_depth 3, min_count 2, 25 %)
    hand = [((4, 4, 0, 0), 0, (1, 1, 2454267026, 1, 0, 0)),      # a tie: the major allele is A; 32/56 of 2^32
            ((4, 4, 0, 0), 1, (1, 1, 2454267026, 1, 1, 0)),      # ... so C differs, but it is in the population
            ((0, 0, 3, 3), 3, (1, 1, 2576980378, 1, 1, 0)),      # the tie G, T: G
            ((6, 2, 0, 0), 1, (1, 1, 1840700270, 1, 1, 0)),      # minor = min_count, 2 / 8 = 25 %: both edges hold
            ((7, 2, 0, 0), 1, (1, 0, 1670265060, 1, 1, 1)),      # 2 / 9 < 25 %
            ((3, 1, 0, 0), 1, (1, 0, 2147483648, 1, 1, 1)),      # 25 % but below min_count
            ((2, 2, 2, 2), 9, (1, 1, 3681400539, 0, 0, 0)),      # r unknown
            ((5, 0, 0, 0), 0, (1, 0, 0, 1, 0, 0)),               # monomorphic: no division
            ((0, 0, 0, 5), 0, (1, 0, 0, 1, 1, 1)),               # a fixed difference
            ((1, 0, 0, 0), 0, (0, 0, 0, 0, 0, 0)),               # n = 1
            ((1, 1, 0, 0), 0, (0, 0, 0, 0, 0, 0)),               # n = 2, below min_depth 3
            ((0, 0, 0, 0), 2, (0, 0, 0, 0, 0, 0)),
            ((2, 0, 1, 0), 4, (1, 0, 2863311531, 0, 0, 0))]      # n = min_depth
    n = len(hand)
    planes = np.zeros((6, n), np.uint32)
    planes[:4] = np.array([h[0] for h in hand]).T
    planes[bm.DEL], planes[bm.N] = 9, 7                          # neither is a base
    ref = np.array([h[1] for h in hand], np.uint8)
    off = begin(bc, [(0, 5, 5 + n)], planes)
    kw = dict(min_depth=3, min_count=2, min_ppm=250000)
    got = check(bc, planes, off, ref=ref, **kw)
    want = np.array([h[2] for h in hand], np.int64).sum(axis=0)
    assert got.rows[0].tolist() == [n, want[0], int(planes[:4].sum()), want[1], want[2], want[3], want[4], want[5]]
    per = dm.per_position(planes, ref=ref, **kw)
    for i, h in enumerate(hand):
        assert per[[1, 3, 4, 5, 6, 7], i].tolist() == list(h[2]), i
    # n = 2 at the default min_depth (0 and 1 act as 2), min_count 0 acts as 1
    for md in (0, 1, 2):
        got = check(bc, planes, off, min_depth=md, min_count=0, ref=ref)
        assert got.rows[0, dm.COVERED] == 11
    check(bc, planes, off, **kw)                                 # and without a reference plane


# ------------------------------------------------------------------- shapes

def test_shapes(bc, P):
    rng = np.random.default_rng(21)
    lens = [1, P - 1, P, P + 1, 2 * P + 1]                       # the one-position segment: later tiles lead by 1..3
    segs, a = [], 0
    for L in lens:
        segs.append((1, a, a + L))
        a += L + 3
    n = sum(lens)
    planes = random_planes(rng, n)
    ref = rng.integers(0, 6, size=n).astype(np.uint8)
    off = begin(bc, segs, planes)
    for window in (0, 16, 17, 100, P - 1, P, P + 1, 3 * P + 5):
        check(bc, planes, off, window, ref=ref, min_depth=3, min_count=2, min_ppm=100000)
    check(bc, planes, off, 16)
    check(bc, planes, off, 0)


def test_window_and_tile_boundaries(bc, P):
    """A window boundary on a tile boundary and one position off it, a
    polymorphic position on each side of both."""
    for lead, window in ((0, P), (0, P - 1), (0, P + 1), (0, P // 2), (1, P - 1), (1, P), (3, 64), (2, 65)):
        segs = ([(0, 0, lead)] if lead else []) + [(0, 10, 10 + 2 * P + 40)]
        n = lead + 2 * P + 40
        planes = np.zeros((6, n), np.uint32)
        planes[bm.A] = 7
        first_tile_end = P                                       # plane index of the second tile's first position
        for i in (first_tile_end - 2, first_tile_end - 1, first_tile_end, first_tile_end + 1, lead + window - 1,
                  lead + window, lead + 2 * window - 1, lead + 2 * window):
            if i < n:
                planes[bm.C, i] = 3 + i % 3
        off = begin(bc, segs, planes)
        got = check(bc, planes, off, window, min_count=2)
        assert got.rows[:, dm.SNV].sum() == np.count_nonzero(planes[bm.C])
        assert (got.rows[:, dm.SNV] > 0).sum() >= 2


def test_segments_empty_duplicated_overlapping(bc, P):
    rng = np.random.default_rng(22)
    segs = [(0, 5, 5), (1, 0, 300), (1, 0, 300), (0, 7, 7), (1, 100, 100 + P), (2, 0, 40), (3, 9, 9)]
    n = sum(b - a for _, a, b in segs)
    planes = random_planes(rng, n)
    ref = rng.integers(0, 5, size=n).astype(np.uint8)
    off = begin(bc, segs, planes)
    for window in (0, 16, 250):
        got = check(bc, planes, off, window, ref=ref)
        assert np.diff(got.win_first)[[0, 3, 6]].tolist() == [0, 0, 0]
    assert check(bc, planes, off, 0).win_first.tolist() == [0, 0, 1, 2, 2, 3, 4, 4]
    off = begin(bc, [])                                          # no segment at all
    got = bc.diversity()
    assert len(got) == 0 and got.win_first.tolist() == [0]
    off = begin(bc, [(0, 3, 3)])
    got = bc.diversity(16)
    assert len(got) == 0 and got.win_first.tolist() == [0, 0]


def test_many_one_position_segments(bc):
    rng = np.random.default_rng(23)
    S = 5000
    planes = random_planes(rng, S)
    ref = rng.integers(0, 5, size=S).astype(np.uint8)
    off = begin(bc, [(int(rng.integers(0, N_REF)), i, i + 1) for i in range(S)], planes)
    for window in (0, 16):
        got = check(bc, planes, off, window, ref=ref)
        assert len(got) == S


def test_more_windows_in_a_tile_than_lanes(bc, P):
    rng = np.random.default_rng(24)
    for lead in (0, 3):
        n = lead + P + P // 2
        planes = random_planes(rng, n, p_mono=0.2, p_empty=0.0)
        segs = ([(0, 0, lead)] if lead else []) + [(2, 1, 1 + n - lead)]
        off = begin(bc, segs, planes)
        got = check(bc, planes, off, 16, ref=rng.integers(0, 4, size=n).astype(np.uint8))
        assert len(got) > 64 and P // 16 > 64


# ------------------------------------------------------------- large counts

def test_large_counts(bc, P):
    lib = bc._lib
    n = 2 * P + 10
    planes = np.zeros((6, n), np.uint32)
    planes[bm.A], planes[bm.C] = 1 << 25, (1 << 25) - 1           # n = 2^26 - 1 everywhere: exact
    planes[bm.C, ::5] = 0
    off = begin(bc, [(0, 0, n)], planes)
    got = check(bc, planes, off, 0)
    assert got.rows[0, dm.PI_FIX] > 1 << 32                       # the pi_fix sum of one window past 2^32
    check(bc, planes, off, 16)
    check(bc, planes, off, P)
    # n = 2^26 at a covered position: MC_E_RANGE naming the index, the lowest of several
    for bad in ([P + 3], [2 * P + 1, 77, P]):
        p2 = planes.copy()
        p2[bm.C, bad] = 1 << 25
        bc.set_counts(0, p2)
        with pytest.raises(_lib.MetacovError) as e:
            bc.diversity(16)
        assert e.value.code == _lib.MC_E_RANGE
        assert re.search(r"plane index (\d+)", str(e.value)).group(1) == str(min(bad))
        out = np.zeros(1, np.int64)
        assert lib.mc_bases_diversity_first(bc._h, _lib.ptr(out)) == _lib.MC_E_STATE    # no result became current
        with pytest.raises(dm.RangeError) as e2:
            dm.diversity_model(p2, off, 16)
        assert e2.value.index == min(bad)
        # the same counts below min_depth are not an error
        p3 = p2.copy()
        p3[:4] = 0
        p3[bm.A, bad] = 1 << 26
        p3[bm.T, bad[0]] = (1 << 32) - 1
        bc.set_counts(0, p3)
        check(bc, p3, off, 16, min_depth=(1 << 33))
        check(bc, p3, off, 0, min_depth=(1 << 33))
    # a bases sum past 2^32 in one window of several tiles (the cross-tile adds are 64-bit)
    p4 = np.zeros((6, n), np.uint32)
    p4[bm.G] = 1 << 22
    p4[bm.T, ::2] = 1 << 22
    bc.set_counts(0, p4)
    got = check(bc, p4, off, 0)
    assert got.rows[0, dm.BASES] > 1 << 32
    got = check(bc, p4, off, 2 * P)
    assert got.rows[0, dm.BASES] > 1 << 32 and got.rows[0, dm.PI_FIX] > 1 << 32


# ---------------------------------------------------------------- reference

def test_reference_plane(bc, P):
    rng = np.random.default_rng(25)
    n = P + 100
    planes = random_planes(rng, n, p_mono=0.3)
    off = begin(bc, [(0, 0, 60), (1, 0, n - 60)], planes)
    ref = (np.arange(n) % 5).astype(np.uint8)                     # A, C, G, T and 4 in turn
    ref[::11] = 255
    ref[5::13] = ord("A")                                         # a letter is not a code
    for window in (0, 16, 40):
        got = check(bc, planes, off, window, ref=ref, min_count=2, min_ppm=300000)
        assert 0 < got.rows[:, dm.COMPARED].sum() < got.rows[:, dm.COVERED].sum()
        assert got.rows[:, dm.POP_DIFF].sum() > 0
        assert (got.rows[:, dm.POP_DIFF] <= got.rows[:, dm.CON_DIFF]).all()
        none = check(bc, planes, off, window, min_count=2, min_ppm=300000)
        assert not none.rows[:, dm.COMPARED:].any()
        assert np.array_equal(none.rows[:, :dm.COMPARED], got.rows[:, :dm.COMPARED])
    for code in range(4):                                         # one class everywhere
        check(bc, planes, off, 16, ref=np.full(n, code, np.uint8))
    got = check(bc, planes, off, 16, ref=np.full(n, 4, np.uint8))
    assert not got.rows[:, dm.COMPARED:].any()
    with pytest.raises(ValueError):
        bc.diversity(ref=ref[:-1])


# -------------------------------------------------------------- cross-checks

def test_against_sites_and_consensus(bc, P):
    rng = np.random.default_rng(26)
    segs = [(0, 0, 700), (1, 50, 50 + P + 30), (2, 0, 1)]
    n = sum(b - a for _, a, b in segs)
    planes = random_planes(rng, n, hi=9, dels=False)
    ref = rng.integers(0, 5, size=n).astype(np.uint8)
    off = begin(bc, segs, planes)
    for md, mc, ppm in ((2, 1, 0), (4, 2, 150000), (3, 1, 400000)):
        got = check(bc, planes, off, 0, min_depth=md, min_count=mc, min_ppm=ppm, ref=ref)
        s = bc.sites(md, mc, ppm)
        assert len(s) > 0 and np.array_equal(got.snv, np.diff(s.first)[np.diff(off) > 0])
        by = check(bc, planes, off, 100, min_depth=md, min_count=mc, min_ppm=ppm, ref=ref)
        for k in range(len(segs)):
            assert by.snv[by.win_first[k]:by.win_first[k + 1]].sum() == s.first[k + 1] - s.first[k]
    got = check(bc, planes, off, 0, min_depth=2, min_count=1, min_ppm=0, ref=ref)
    c = bc.consensus(min_depth=2, call_ppm=0, min_count=1, ref=ref)
    assert np.array_equal(got.con_diff, c.summary[:, mb.DIFFERS]) and got.con_diff.sum() > 0


# --------------------------------------------------------- state and errors

def _code(call):
    try:
        call()
    except _lib.MetacovError as e:
        return e.code
    return 0


def test_state_and_errors(P):
    lib = _lib.load()
    rng = np.random.default_rng(27)
    with mb.BaseCounter(N_REF, 0) as h:
        one, f32 = np.zeros(8, np.int64), ctypes.c_float()
        dp, dn = ctypes.c_void_p(), ctypes.c_int64()
        raw = {"first": lambda: _lib.check(lib.mc_bases_diversity_first(h._h, _lib.ptr(one)), lib),
               "get": lambda: _lib.check(lib.mc_bases_diversity_get(h._h, 0, 0, None), lib),
               "device": lambda: _lib.check(lib.mc_bases_diversity_device(h._h, ctypes.byref(dp), ctypes.byref(dn)),
                                            lib),
               "timing": lambda: _lib.check(lib.mc_bases_diversity_timing(h._h, ctypes.byref(f32),
                                                                          ctypes.byref(f32)), lib)}
        assert _code(lambda: h.diversity()) == _lib.MC_E_STATE                 # before begin
        for call in raw.values():
            assert _code(call) == _lib.MC_E_STATE
        n = P + 50
        planes = random_planes(rng, n)
        h.begin([0, 1], [0, 0], [40, n - 40])
        h.set_counts(0, planes)
        for call in raw.values():
            assert _code(call) == _lib.MC_E_STATE
        for kw in (dict(min_depth=-1), dict(min_count=-1), dict(min_ppm=-1), dict(min_ppm=1000001), dict(window=1),
                   dict(window=15), dict(window=-16)):
            assert _code(lambda: h.diversity(**kw)) == _lib.MC_E_INVALID, kw
        for call in raw.values():
            assert _code(call) == _lib.MC_E_STATE
        d = h.diversity(16, min_ppm=1000000)
        first, rows = dm.diversity_model(planes, h.seg_off, 16, min_ppm=1000000)
        assert np.array_equal(d.rows, rows)
        for call in raw.values():
            call()
        assert dn.value == len(rows) and dp.value
        t = h.diversity_timing()
        assert t["tile_ms"] > 0 and t["combine_ms"] >= 0
        for f, c in ((-1, 1), (0, len(rows) + 1), (len(rows), 1), (len(rows) + 1, 0), (0, -1)):
            assert lib.mc_bases_diversity_get(h._h, f, c, _lib.ptr(np.zeros(8 * (len(rows) + 2), np.int64))) == \
                _lib.MC_E_INVALID
        assert lib.mc_bases_diversity_get(h._h, len(rows), 0, None) == 0
        assert lib.mc_bases_diversity_get(h._h, 0, 1, None) == _lib.MC_E_INVALID
        part = np.zeros((2, 8), np.int64)
        _lib.check(lib.mc_bases_diversity_get(h._h, 1, 2, _lib.ptr(part)), lib)
        assert np.array_equal(part, rows[1:3])
        # two calls in a row give equal rows
        assert np.array_equal(h.diversity(16, min_ppm=1000000).rows, rows)
        # sites and a consensus survive a diversity call, and the other way round
        ref = rng.integers(0, 5, size=n).astype(np.uint8)
        s = h.sites(2, 1, 0)
        c = h.consensus(min_depth=2, ref=ref)
        letters = h.consensus_letters(False, 0, n)
        d = h.diversity(100, ref=ref)
        first, rows = dm.diversity_model(planes, h.seg_off, 100, ref=ref)
        assert np.array_equal(d.rows, rows)
        pos, cnt = np.zeros(len(s), np.int64), np.zeros((len(s), 6), np.uint32)
        _lib.check(lib.mc_bases_sites_get(h._h, 0, len(s), _lib.ptr(pos), _lib.ptr(cnt)), lib)
        assert len(s) > 0 and np.array_equal(pos, s.pos) and np.array_equal(cnt, s.counts)
        assert np.array_equal(h.consensus_letters(False, 0, n), letters)
        h.sites(3, 2, 0, ref=ref)
        h.consensus(iupac=True)
        got = np.zeros_like(rows)
        _lib.check(lib.mc_bases_diversity_get(h._h, 0, len(rows), _lib.ptr(got)), lib)
        assert np.array_equal(got, rows)
        # set_counts, add_reads and begin drop it
        h.set_counts(3, np.zeros((6, 2), np.uint32))
        for call in raw.values():
            assert _code(call) == _lib.MC_E_STATE
        planes[:, 3:5] = 0
        assert np.array_equal(h.diversity(16).rows, dm.diversity_model(planes, h.seg_off, 16)[1])
        h.add_reads(*bm.batch_args(bm.make_batch([(0, 1, "2M", "CG", 30)])))
        for call in raw.values():
            assert _code(call) == _lib.MC_E_STATE
        planes[bm.C, 1] += 1
        planes[bm.G, 2] += 1
        assert np.array_equal(h.diversity(16).rows, dm.diversity_model(planes, h.seg_off, 16)[1])
        raw["get"]()
        h.begin([0], [0], [4])
        for call in raw.values():
            assert _code(call) == _lib.MC_E_STATE
        # an installed insertion table drops it as the consensus
        h.begin([0], [0], [20], insertions=True)
        h.diversity()
        raw["first"]()
        h.set_insertions([2], [1], [0], [0], [1])
        for call in raw.values():
            assert _code(call) == _lib.MC_E_STATE


# --------------------------------------------------------------- end to end

@pytest.mark.parametrize("seed", range(20))
def test_fuzz_through_pileup(bc, P, seed):
    rng = np.random.default_rng(900 + seed)
    L = 2 * P + int(rng.integers(0, 50))
    reads = []
    for _ in range(int(rng.integers(30, 90))):
        c = random_cigar(rng, P)
        n = bm.query_length(bm.cigar_words(c))
        reads.append((int(rng.integers(0, 2)), int(rng.integers(0, L)), c,
                      rng.choice([1, 2, 4, 8, 15], size=n, p=[.3, .3, .18, .18, .04]).tolist(), 30))
    segs = []
    for _ in range(int(rng.integers(1, 6))):
        a = int(rng.integers(0, L))
        segs.append((int(rng.integers(0, 2)), a, a + int(rng.integers(0, L))))
    b = bm.make_batch(sorted(reads, key=lambda r: (r[0], r[1])))
    tids, starts, ends = (np.array(x, np.int64) for x in zip(*segs))
    off, planes = bm.counts_model(b, tids, starts, ends)
    ref = rng.integers(0, 5, size=planes.shape[1]).astype(np.uint8) if seed % 2 else None
    kw = dict(min_depth=int(rng.integers(0, 5)), min_count=int(rng.integers(0, 3)),
              min_ppm=int(rng.integers(0, 500000)), ref=ref)
    window = int(rng.choice([0, 16, 33, 500, P]))
    bc.begin(tids, starts, ends)
    bc.add_reads(*bm.batch_args(b))
    plain = check(bc, planes, off, window, **kw)
    flags = rng.choice([0, 0x10], size=bm.n_reads(b)).astype(np.uint16)
    bc.begin(tids, starts, ends, strand=True)
    bc.add_reads(*bm.batch_args(b), flag=flags)
    stranded = check(bc, planes, off, window, **kw)
    assert np.array_equal(plain.rows, stranded.rows)


DIV_VARIANTS = {
    "whole": ([], dict(), 0, False, False),
    "whole_ref": (["-f", "FA", "--min-depth", "3", "--min-count", "1", "--min-frac", "0.2"],
                  dict(min_depth=3, min_count=1, min_ppm=200000), 0, True, False),
    "by100_ref": (["--by", "100", "-f", "FA", "--min-depth", "2"], dict(min_depth=2), 100, True, False),
    "by100": (["--by", "100", "--min-depth", "0", "--min-count", "0", "--min-frac", "0"],
              dict(min_depth=0, min_count=0, min_ppm=0), 100, False, False),
    "regions_whole_ref": (["-rc", "RC", "-f", "FA", "--min-depth", "2"], dict(min_depth=2), 0, True, True),
    "regions_by100": (["-rc", "RC", "--by", "100"], dict(), 100, False, True),
}
CLI_DEFAULTS = dict(min_depth=5, min_count=2, min_ppm=50000)


@pytest.mark.parametrize("variant", sorted(DIV_VARIANTS))
@pytest.mark.parametrize("name", ["bbmap.sorted.bam", "synth_exp.bam"])
def test_cli(golden_dir, tmp_path, name, variant):
    from metacov_amd.cli import main
    g = golden(golden_dir, name)
    path, fa, names, lengths = g[:4]
    args, kw, window, use_ref, with_regions = DIV_VARIANTS[variant]
    kw = dict(CLI_DEFAULTS, **kw)
    big = int(np.argmax(lengths))
    if with_regions:
        regs = [(big, 5, min(lengths[big], 700)), (0, 0, lengths[0]), (big, lengths[big] - 20, lengths[big] + 15),
                (big, 5, min(lengths[big], 700))]
        rc = tmp_path / "r.csv"
        rc.write_text("sequence_id,start,stop\n" + "".join("%s,%d,%d\n" % (names[t], a, b) for t, a, b in regs))
    else:
        regs = [(t, 0, L) for t, L in enumerate(lengths)]
    planes, codes, seg_off = region_planes(g, regs)
    first, rows = dm.diversity_model(planes, seg_off, window, ref=codes if use_ref else None, **kw)
    want = dm.tsv([names[t] for t, _, _ in regs], [a for _, a, _ in regs], seg_off, window, first, rows)
    args = [fa if a == "FA" else str(tmp_path / "r.csv") if a == "RC" else a for a in args]
    texts = []
    for decode in ("host", "gpu"):
        out = tmp_path / ("%s.tsv" % decode)
        r = CliRunner().invoke(main, ["diversity", "-b", path, "-o", str(out), "--decode", decode] + args)
        assert r.exit_code == 0, r.output
        texts.append(out.read_text())
    assert texts[0] == texts[1]
    assert texts[0] == want
    assert rows[:, dm.BASES].sum() > 0
    if use_ref:
        assert rows[:, dm.COMPARED].sum() > 0
    else:
        assert all(line.endswith("\tNA\tNA") for line in want.splitlines()[1:])
    # and the writer over the model gives these bytes
    fh = io.StringIO()
    mb.write_diversity(fh, [names[t] for t, _, _ in regs], [a for _, a, _ in regs], mb.Diversity(first, rows, window))
    assert fh.getvalue() == want


def test_diversity_convenience(golden_dir):
    g = golden(golden_dir, "bbmap.sorted.bam")
    path, fa, names, lengths, b, seqs = g
    t = int(np.argmax(lengths))
    a, e = 10, lengths[t] // 2
    p, codes, seg_off = region_planes(g, [(t, a, e)])
    ref = (seqs.get(names[t], "") + "N" * e)[a:e]
    first, rows = dm.diversity_model(p, seg_off, 64, ref=codes, min_depth=3)
    for decode in ("host", "gpu"):
        got = mb.diversity(path, names[t], a, e, window=64, min_depth=3, ref=ref, decode=decode)
        assert np.array_equal(got.rows, rows) and np.array_equal(got.win_first, first)
    with pytest.raises(KeyError):
        mb.diversity(path, "no_such_contig")
    with pytest.raises(ValueError):
        mb.diversity(path, names[t], 0, 10, ref="ACGT")
