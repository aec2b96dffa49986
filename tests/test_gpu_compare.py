"""Sample comparison on the GPU (csrc/bases_cmp.h) against the model in
tests/compare_model.py: exact equality of win_first and of every row.  Planes
are set through set_counts (mc_bases_set) on two counters except in the
end-to-end tests; shapes are a few tiles at most; P (tile positions) comes
from the library."""
import ctypes
import io
import re

import numpy as np
import pytest
from click.testing import CliRunner

from metacov_amd import _lib
from metacov_amd import bases as mb
from metacov_amd import synth
from tests import bases_model as bm
from tests import compare_model as cm
from tests import diversity_model as dm
from tests.test_compare import one_hot_reference, random_pair
from tests.test_gpu_consensus import random_cigar

pytestmark = pytest.mark.gpu

N_REF = 4


@pytest.fixture(scope="module")
def a(lib_built):
    h = mb.BaseCounter(N_REF, 0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def b(lib_built):
    h = mb.BaseCounter(N_REF, 0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def P(lib_built):
    return mb.dims()


def begin(h, segs, planes=None, **kw):
    tids, starts, ends = (np.array(x, np.int64) for x in zip(*segs)) if segs else (np.zeros(0, np.int64),) * 3
    n = h.begin(tids, starts, ends, **kw)
    if planes is not None:
        assert planes.shape == (6, n)
        h.set_counts(0, planes)
    return h.seg_off


def begin_both(a, b, segs, pa=None, pb=None):
    off = begin(a, segs, pa)
    assert np.array_equal(begin(b, segs, pb), off)
    return off


def check(a, b, pa, pb, seg_off, window=0, **kw):
    got = a.compare(b, window, **kw)
    first, rows = cm.compare_model(pa, pb, seg_off, window, **kw)
    assert got.rows.dtype == np.int64 and got.rows.shape == rows.shape
    assert np.array_equal(got.win_first, first)
    bad = np.argwhere(got.rows != rows)
    assert len(bad) == 0, "window %d: rows differ first at (row, column) %s: got %s, want %s" % (
        window, bad[0], got.rows[bad[0][0]], rows[bad[0][0]])
    assert got.rows[:, cm.POSITIONS].sum() == pa.shape[1]
    return got


def _code(call):
    try:
        call()
    except _lib.MetacovError as e:
        return e.code
    return 0


# --------------------------------------------------------------------- rule

HALF, ONE = 1 << 31, 1 << 32

#        sample a       sample b       covered_a covered_b compared con pop snv q   (min_depth 3, min_count 2, 25 %)
HAND = [((4, 4, 0, 0), (4, 4, 0, 0), (1, 1, 1, 0, 0, 1, 0)),              # a tie in both: A and A; proportional
        ((4, 4, 0, 0), (0, 5, 0, 0), (1, 1, 1, 1, 0, 1, HALF)),           # a tie in a: A, but b's C is present in a
        ((0, 0, 0, 6), (0, 0, 3, 3), (1, 1, 1, 1, 0, 1, HALF)),           # a tie in b: G, but a's T is present in b
        ((6, 2, 0, 0), (0, 8, 0, 0), (1, 1, 1, 1, 0, 1, 3221225472)),     # C in a: min_count and 2 / 8 = 25 %, both edges
        ((7, 2, 0, 0), (0, 9, 0, 0), (1, 1, 1, 1, 1, 0, 3340530119)),     # 2 / 9 < 25 %: C is not in a
        ((6, 0, 2, 0), (0, 7, 2, 0), (1, 1, 1, 1, 1, 1, 3340530119)),     # G = 2 qualifies in a, fails in the deeper b
        ((7, 0, 2, 0), (0, 7, 2, 0), (1, 1, 1, 1, 1, 0, 3340530119)),     # ... and in neither
        ((6, 2, 0, 0), (2, 6, 0, 0), (1, 1, 1, 1, 0, 1, HALF)),           # other majors, a's major is present in b
        ((5, 0, 0, 0), (0, 0, 0, 5), (1, 1, 1, 1, 1, 0, ONE)),            # fully disjoint alleles
        ((5, 0, 0, 0), (1, 1, 0, 0), (1, 0, 0, 0, 0, 0, 0)),              # covered in a only
        ((0, 0, 0, 0), (0, 3, 0, 0), (0, 1, 0, 0, 0, 0, 0)),              # covered in b only
        ((2, 0, 1, 0), (2, 1, 0, 0), (1, 1, 1, 0, 0, 0, 1431655765)),     # n = min_depth in both; the minors below min_count
        ((1, 0, 0, 0), (0, 0, 1, 0), (0, 0, 0, 0, 0, 0, 0)),              # n = 1
        ((0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 0)),              # both empty
        ((1, 1, 0, 0), (1, 1, 0, 0), (0, 0, 0, 0, 0, 0, 0)),              # n = 2, below min_depth 3
        ((5, 0, 0, 0), (9, 0, 0, 0), (1, 1, 1, 0, 0, 0, 0))]              # the same single allele: no division


def test_rule_by_hand(a, b):
    n = len(HAND)
    pa, pb = np.zeros((6, n), np.uint32), np.zeros((6, n), np.uint32)
    pa[:4] = np.array([h[0] for h in HAND]).T
    pb[:4] = np.array([h[1] for h in HAND]).T
    pa[bm.DEL], pa[bm.N], pb[bm.DEL], pb[bm.N] = 9, 7, 11, 100            # neither is a base
    off = begin_both(a, b, [(0, 5, 5 + n)], pa, pb)
    kw = dict(min_depth=3, min_count=2, min_ppm=250000)
    got = check(a, b, pa, pb, off, **kw)
    want = np.array([h[2] for h in HAND], np.int64).sum(axis=0)
    assert got.rows[0].tolist() == [n] + want.tolist()
    per = cm.per_position(pa, pb, **kw)
    for i, h in enumerate(HAND):
        assert per[1:, i].tolist() == list(h[2]), i
    # n = 2 at the default min_depth (0 and 1 act as 2), min_count 0 acts as 1
    for md in (0, 1, 2):
        got = check(a, b, pa, pb, off, min_depth=md, min_count=0)
        # a lacks 2 bases at three positions (n = 0, 1, 0), b at two of them (n = 1, 0)
        assert got.rows[0, 1:4].tolist() == [13, 14, 13]


# ------------------------------------------------------------------- shapes

def test_shapes(a, b, P):
    rng = np.random.default_rng(31)
    lens = [1, P - 1, P, P + 1, 2 * P + 1]                       # the one-position segment: later tiles lead by 1..3
    segs, x = [], 0
    for L in lens:
        segs.append((1, x, x + L))
        x += L + 3
    n = sum(lens)
    pa, pb = random_pair(rng, n, mc=2, ppm=100000)
    off = begin_both(a, b, segs, pa, pb)
    for window in (0, 16, 17, 100, P - 1, P, P + 1, 3 * P + 5):
        check(a, b, pa, pb, off, window, min_depth=3, min_count=2, min_ppm=100000)
    check(a, b, pa, pb, off, 16)
    check(a, b, pa, pb, off, 0)


def test_window_and_tile_boundaries(a, b, P):
    """A window boundary on a tile boundary and one position off it, a
    differing position on each side of both."""
    for lead, window in ((0, P), (0, P - 1), (0, P + 1), (0, P // 2), (1, P - 1), (1, P), (3, 64), (2, 65)):
        segs = ([(0, 0, lead)] if lead else []) + [(0, 10, 10 + 2 * P + 40)]
        n = lead + 2 * P + 40
        pa, pb = np.zeros((6, n), np.uint32), np.zeros((6, n), np.uint32)
        pa[bm.A], pb[bm.A] = 7, 5
        marks = [i for i in (P - 2, P - 1, P, P + 1, lead + window - 1, lead + window, lead + 2 * window - 1,
                             lead + 2 * window) if i < n]        # P: the second tile's first plane index
        for i in marks:
            pb[bm.A, i], pb[bm.C, i] = 0, 3 + i % 3
        off = begin_both(a, b, segs, pa, pb)
        got = check(a, b, pa, pb, off, window, min_count=2)
        assert got.rows[:, cm.POP_DIFF].sum() == got.rows[:, cm.CON_DIFF].sum() == len(set(marks))
        assert got.rows[:, cm.DIST_FIX].sum() == len(set(marks)) * ONE
        assert (got.rows[:, cm.CON_DIFF] > 0).sum() >= 2


def test_segments_empty_duplicated_overlapping(a, b, P):
    rng = np.random.default_rng(32)
    segs = [(0, 5, 5), (1, 0, 300), (1, 0, 300), (0, 7, 7), (1, 100, 100 + P), (2, 0, 40), (3, 9, 9)]
    n = sum(z - x for _, x, z in segs)
    pa, pb = random_pair(rng, n)
    off = begin_both(a, b, segs, pa, pb)
    for window in (0, 16, 250):
        got = check(a, b, pa, pb, off, window)
        assert np.diff(got.win_first)[[0, 3, 6]].tolist() == [0, 0, 0]
    assert check(a, b, pa, pb, off, 0).win_first.tolist() == [0, 0, 1, 2, 2, 3, 4, 4]
    begin_both(a, b, [])                                         # no segment at all
    got = a.compare(b)
    assert len(got) == 0 and got.win_first.tolist() == [0]
    begin_both(a, b, [(0, 3, 3)])
    got = a.compare(b, 16)
    assert len(got) == 0 and got.win_first.tolist() == [0, 0]


def test_many_one_position_segments(a, b):
    rng = np.random.default_rng(33)
    S = 5000
    pa, pb = random_pair(rng, S)
    off = begin_both(a, b, [(int(rng.integers(0, N_REF)), i, i + 1) for i in range(S)], pa, pb)
    for window in (0, 16):
        got = check(a, b, pa, pb, off, window)
        assert len(got) == S


def test_more_windows_in_a_tile_than_lanes(a, b, P):
    rng = np.random.default_rng(34)
    for lead in (0, 3):
        n = lead + P + P // 2
        pa, pb = random_pair(rng, n)
        segs = ([(0, 0, lead)] if lead else []) + [(2, 1, 1 + n - lead)]
        off = begin_both(a, b, segs, pa, pb)
        got = check(a, b, pa, pb, off, 16)
        assert len(got) > 128 and P // 16 >= 128                 # 128 windows inside the first tile


def test_unequal_buffers(a, P):
    """b's grow-only buffers come from a much larger begin: its planes pointer
    differs from a's in everything but the layout of the segments in use."""
    rng = np.random.default_rng(35)
    with mb.BaseCounter(N_REF, 0) as big:
        begin(big, [(0, 0, 40 * P + 7), (1, 0, 3 * P)])
        segs = [(0, 2, 3), (1, 0, P + 9), (2, 4, 4 + 70)]
        n = sum(z - x for _, x, z in segs)
        pa, pb = random_pair(rng, n)
        off = begin(a, segs, pa)
        assert np.array_equal(begin(big, segs, pb), off)
        for window in (0, 16, 100):
            check(a, big, pa, pb, off, window, min_depth=3, min_count=2, min_ppm=250000)
            check(big, a, pb, pa, off, window, min_depth=3, min_count=2, min_ppm=250000)


def test_self_comparison(a, P):
    rng = np.random.default_rng(36)
    n = 2 * P + 11
    pa, _ = random_pair(rng, n)
    off = begin(a, [(0, 0, 5), (1, 0, n - 5)], pa)
    for window in (0, 16, 300):
        got = check(a, a, pa, pa, off, window, min_depth=3)
        assert not got.rows[:, [cm.CON_DIFF, cm.POP_DIFF, cm.DIST_FIX]].any()
        assert np.array_equal(got.compared, got.covered_a) and np.array_equal(got.compared, got.covered_b)
        assert got.compared.sum() > 0 and got.snv.sum() > 0


def test_symmetry(a, b, P):
    rng = np.random.default_rng(37)
    n = 2 * P + 77
    pa, pb = random_pair(rng, n, hi=40)
    off = begin_both(a, b, [(0, 0, 3), (3, 50, 50 + n - 3)], pa, pb)
    for window, kw in ((0, dict()), (16, dict(min_depth=4, min_count=2, min_ppm=250000)), (P, dict(min_depth=3))):
        ab = check(a, b, pa, pb, off, window, **kw)
        ba = check(b, a, pb, pa, off, window, **kw)
        assert np.array_equal(ab.rows[:, [0, 2, 1, 3, 4, 5, 6, 7]], ba.rows)
        assert ab.dist_fix.any() and (ab.covered_a != ab.covered_b).any()


def test_reduction_to_diversity(a, b, P):
    """b shows the reference base min_depth times where its code is known:
    compared, con_diff and pop_diff are the diversity call's against that
    reference, both computed on the device."""
    rng = np.random.default_rng(38)
    n = P + 300
    pa, _ = random_pair(rng, n)
    ref = rng.integers(0, 6, size=n).astype(np.uint8)
    segs = [(0, 0, 1), (1, 0, n - 1)]
    for kw in (dict(), dict(min_depth=3, min_count=2, min_ppm=250000), dict(min_depth=5, min_ppm=400000)):
        pb = one_hot_reference(ref, max(kw.get("min_depth", 2), 2))
        off = begin_both(a, b, segs, pa, pb)
        for window in (0, 16, 100):
            got = check(a, b, pa, pb, off, window, **kw)
            div = a.diversity(window, ref=ref, **kw)
            assert np.array_equal(got.win_first, div.win_first)
            assert np.array_equal(got.rows[:, [cm.COMPARED, cm.CON_DIFF, cm.POP_DIFF]],
                                  div.rows[:, [dm.COMPARED, dm.CON_DIFF, dm.POP_DIFF]])
            assert div.pop_diff.sum() > 0 and div.con_diff.sum() > div.pop_diff.sum()


# ------------------------------------------------------------- large counts

def test_large_counts(a, b, P):
    lib = a._lib
    n = 2 * P + 10
    pa, pb = np.zeros((6, n), np.uint32), np.zeros((6, n), np.uint32)
    pa[bm.A], pa[bm.C] = 1 << 25, (1 << 25) - 1                    # n = 2^26 - 1 everywhere in both: exact
    pb[bm.C], pb[bm.T] = (1 << 25) - 1, 1 << 25
    pb[bm.T, ::5], pb[bm.G, ::5] = 0, 1 << 25
    off = begin_both(a, b, [(0, 0, n)], pa, pb)
    got = check(a, b, pa, pb, off, 0)
    assert got.rows[0, cm.DIST_FIX] > 1 << 32 and got.rows[0, cm.COMPARED] == n
    check(a, b, pa, pb, off, 16)
    check(a, b, pa, pb, off, P)
    # n = 2^26 at a compared position: MC_E_RANGE naming the index, the lowest of several, in a only and in b only
    for which in (0, 1):
        for bad in ([P + 3], [2 * P + 1, 77, P]):
            qa, qb = pa.copy(), pb.copy()
            (qa, qb)[which][bm.C, bad] = 1 << 25
            a.set_counts(0, qa)
            b.set_counts(0, qb)
            with pytest.raises(_lib.MetacovError) as e:
                a.compare(b, 16)
            assert e.value.code == _lib.MC_E_RANGE
            assert re.search(r"plane index (\d+)", str(e.value)).group(1) == str(min(bad))
            out = np.zeros(2, np.int64)
            assert lib.mc_bases_compare_first(a._h, _lib.ptr(out)) == _lib.MC_E_STATE      # no result became current
            with pytest.raises(cm.RangeError) as e2:
                cm.compare_model(qa, qb, off, 16)
            assert e2.value.index == min(bad)
            # the other sample uncovered there: not compared, not an error
            other = (qb, qa)[which]
            other[:4, bad] = 0
            other[bm.G, bad[0]] = 1
            (qa, qb)[which][bm.T, bad[0]] = (1 << 32) - 1
            a.set_counts(0, qa)
            b.set_counts(0, qb)
            got = check(a, b, qa, qb, off, 16)
            assert got.compared.sum() == n - len(bad)
            check(a, b, qa, qb, off, 0)
    # a dist_fix sum past 2^32 in one window of two tiles (the cross-tile adds are 64-bit)
    qa, qb = np.zeros((6, n), np.uint32), np.zeros((6, n), np.uint32)
    qa[bm.G], qb[bm.T] = 1 << 22, 3
    a.set_counts(0, qa)
    b.set_counts(0, qb)
    got = check(a, b, qa, qb, off, 2 * P)
    assert got.rows[0, cm.DIST_FIX] == 2 * P * ONE and got.rows[0, cm.POP_DIFF] == 2 * P


# --------------------------------------------------------- state and errors

def test_state_and_errors(P):
    lib = _lib.load()
    rng = np.random.default_rng(39)
    with mb.BaseCounter(N_REF, 0) as h, mb.BaseCounter(N_REF, 0) as o:
        one, f32 = np.zeros(8, np.int64), ctypes.c_float()
        dp, dn = ctypes.c_void_p(), ctypes.c_int64()
        raw = {"first": lambda: _lib.check(lib.mc_bases_compare_first(h._h, _lib.ptr(one)), lib),
               "get": lambda: _lib.check(lib.mc_bases_compare_get(h._h, 0, 0, None), lib),
               "device": lambda: _lib.check(lib.mc_bases_compare_device(h._h, ctypes.byref(dp), ctypes.byref(dn)),
                                            lib),
               "timing": lambda: _lib.check(lib.mc_bases_compare_timing(h._h, ctypes.byref(f32),
                                                                        ctypes.byref(f32)), lib)}

        def stale():
            return all(_code(call) == _lib.MC_E_STATE for call in raw.values())

        n = P + 50
        segs = ([0, 1], [0, 0], [40, n - 40])
        pa, pb = random_pair(rng, n)
        assert _code(lambda: h.compare(o)) == _lib.MC_E_STATE                  # neither begun
        h.begin(*segs)
        h.set_counts(0, pa)
        assert _code(lambda: h.compare(o)) == _lib.MC_E_STATE                  # only a begun
        assert _code(lambda: o.compare(h)) == _lib.MC_E_STATE                  # only b begun
        assert stale()
        nw = ctypes.c_int64()
        assert lib.mc_bases_compare(h._h, None, 0, 2, 1, 0, ctypes.byref(nw)) == _lib.MC_E_INVALID
        assert lib.mc_bases_compare(None, h._h, 0, 2, 1, 0, ctypes.byref(nw)) == _lib.MC_E_INVALID
        assert lib.mc_bases_compare(h._h, h._h, 0, 2, 1, 0, None) == _lib.MC_E_INVALID
        with pytest.raises(TypeError):
            h.compare(None)
        # differing segments: the first one is named
        for other, which in ((([0, 1, 1], [0, 0, 0], [40, n - 40, 5]), 2), (([0, 1], [0, 0], [40, n - 41]), 1),
                             (([2, 1], [0, 0], [40, n - 40]), 0), (([0, 1], [1, 0], [41, n - 40]), 0),
                             (([0], [0], [40]), 1)):
            o.begin(*other)
            with pytest.raises(_lib.MetacovError) as e:
                h.compare(o)
            assert e.value.code == _lib.MC_E_INVALID and "segment %d" % which in str(e.value), str(e.value)
        assert stale()
        o.begin(*segs)
        o.set_counts(0, pb)
        for kw in (dict(min_depth=-1), dict(min_count=-1), dict(min_ppm=-1), dict(min_ppm=1000001), dict(window=1),
                   dict(window=15), dict(window=-16)):
            assert _code(lambda: h.compare(o, **kw)) == _lib.MC_E_INVALID, kw
        assert stale()
        d = h.compare(o, 16, min_ppm=1000000)
        first, rows = cm.compare_model(pa, pb, h.seg_off, 16, min_ppm=1000000)
        assert np.array_equal(d.rows, rows) and np.array_equal(d.win_first, first)
        for call in raw.values():
            call()
        assert dn.value == len(rows) and dp.value
        t = h.compare_timing()
        assert t["tile_ms"] > 0 and t["zero_ms"] >= 0
        for f, c in ((-1, 1), (0, len(rows) + 1), (len(rows), 1), (len(rows) + 1, 0), (0, -1)):
            assert lib.mc_bases_compare_get(h._h, f, c, _lib.ptr(np.zeros(8 * (len(rows) + 2), np.int64))) == \
                _lib.MC_E_INVALID
        assert lib.mc_bases_compare_get(h._h, len(rows), 0, None) == 0
        assert lib.mc_bases_compare_get(h._h, 0, 1, None) == _lib.MC_E_INVALID
        part = np.zeros((2, 8), np.int64)
        _lib.check(lib.mc_bases_compare_get(h._h, 1, 2, _lib.ptr(part)), lib)
        assert np.array_equal(part, rows[1:3])
        assert _code(lambda: _lib.check(lib.mc_bases_compare_first(o._h, _lib.ptr(one)), lib)) == _lib.MC_E_STATE
        assert np.array_equal(h.compare(o, 16, min_ppm=1000000).rows, rows)     # two calls in a row

        def current():
            got = np.zeros_like(rows)
            _lib.check(lib.mc_bases_compare_get(h._h, 0, len(rows), _lib.ptr(got)), lib)
            return got

        # sites, consensus and diversity on both handles live across a compare, and the other way round
        ref = rng.integers(0, 5, size=n).astype(np.uint8)
        kept = []
        for x, p in ((h, pa), (o, pb)):
            s = x.sites(2, 1, 0)
            x.consensus(min_depth=2, ref=ref)
            dv = x.diversity(100, ref=ref)
            kept.append((s, x.consensus_letters(False, 0, n), dv.rows.copy()))
            assert np.array_equal(dv.rows, dm.diversity_model(p, x.seg_off, 100, ref=ref)[1])
        assert np.array_equal(current(), rows)
        assert np.array_equal(h.compare(o, 16, min_ppm=1000000).rows, rows)
        for x, (s, letters, div_rows) in zip((h, o), kept):
            pos, cnt = np.zeros(len(s), np.int64), np.zeros((len(s), 6), np.uint32)
            _lib.check(lib.mc_bases_sites_get(x._h, 0, len(s), _lib.ptr(pos), _lib.ptr(cnt)), lib)
            assert len(s) > 0 and np.array_equal(pos, s.pos) and np.array_equal(cnt, s.counts)
            assert np.array_equal(x.consensus_letters(False, 0, n), letters)
            got = np.zeros_like(div_rows)
            _lib.check(lib.mc_bases_diversity_get(x._h, 0, len(div_rows), _lib.ptr(got)), lib)
            assert np.array_equal(got, div_rows)
        # calls on b do not touch a's result: its rows stay those of the planes b had
        o.set_counts(3, np.zeros((6, 2), np.uint32))
        o.add_reads(*bm.batch_args(bm.make_batch([(0, 1, "2M", "CG", 30)])))
        assert np.array_equal(current(), rows)
        o.begin([0], [0], [4])
        assert np.array_equal(current(), rows)
        o.begin(*segs)
        o.set_counts(0, pb)
        # a's set_counts, add_reads and begin drop it
        h.set_counts(3, np.zeros((6, 2), np.uint32))
        assert stale()
        pa[:, 3:5] = 0
        assert np.array_equal(h.compare(o, 16).rows, cm.compare_model(pa, pb, h.seg_off, 16)[1])
        h.add_reads(*bm.batch_args(bm.make_batch([(0, 1, "2M", "CG", 30)])))
        assert stale()
        pa[bm.C, 1] += 1
        pa[bm.G, 2] += 1
        assert np.array_equal(h.compare(o, 16).rows, cm.compare_model(pa, pb, h.seg_off, 16)[1])
        raw["get"]()
        h.begin([0], [0], [4])
        assert stale()
        # an installed insertion table drops it as the consensus and the diversity
        h.begin([0], [0], [20], insertions=True)
        o.begin([0], [0], [20])
        h.compare(o)
        raw["first"]()
        h.set_insertions([2], [1], [0], [0], [1])
        assert stale()


# --------------------------------------------------------------- end to end

def _reads(rng, P, L):
    reads = []
    for _ in range(int(rng.integers(30, 90))):
        c = random_cigar(rng, P)
        n = bm.query_length(bm.cigar_words(c))
        reads.append((int(rng.integers(0, 2)), int(rng.integers(0, L)), c,
                      rng.choice([1, 2, 4, 8, 15], size=n, p=[.3, .3, .18, .18, .04]).tolist(), 30))
    return bm.make_batch(sorted(reads, key=lambda r: (r[0], r[1])))


@pytest.mark.parametrize("seed", range(10))
def test_fuzz_through_pileup(a, b, P, seed):
    rng = np.random.default_rng(1200 + seed)
    L = 2 * P + int(rng.integers(0, 50))
    ba, bb = _reads(rng, P, L), _reads(rng, P, L)
    segs = []
    for _ in range(int(rng.integers(1, 6))):
        x = int(rng.integers(0, L))
        segs.append((int(rng.integers(0, 2)), x, x + int(rng.integers(0, L))))
    tids, starts, ends = (np.array(x, np.int64) for x in zip(*segs))
    off, pa = bm.counts_model(ba, tids, starts, ends)
    _, pb = bm.counts_model(bb, tids, starts, ends)
    kw = dict(min_depth=int(rng.integers(0, 5)), min_count=int(rng.integers(0, 3)),
              min_ppm=int(rng.integers(0, 500000)))
    window = int(rng.choice([0, 16, 33, 500, P]))
    a.begin(tids, starts, ends)
    a.add_reads(*bm.batch_args(ba))
    b.begin(tids, starts, ends)
    b.add_reads(*bm.batch_args(bb))
    plain = check(a, b, pa, pb, off, window, **kw)
    if seed == 0:                                                 # strand tracking on b does not change a row
        flags = rng.choice([0, 0x10], size=bm.n_reads(bb)).astype(np.uint16)
        b.begin(tids, starts, ends, strand=True)
        b.add_reads(*bm.batch_args(bb), flag=flags)
        assert np.array_equal(check(a, b, pa, pb, off, window, **kw).rows, plain.rows)


NAMES, BASES = ["ctg_1", "ctg_2"], "ACGT"


@pytest.fixture(scope="module")
def two_bams(tmp_path_factory, P):
    """Two BAMs with one header: two contigs of about 2P + 50 positions, each
    sample's reads carrying a base mix of its own."""
    d = tmp_path_factory.mktemp("compare")
    lengths = [2 * P + 50, 2 * P + 37]
    out = []
    for k, seed in enumerate((71, 72)):
        rng = np.random.default_rng(seed)
        recs = []
        for tid, L in enumerate(lengths):
            for i in range(260):
                n = int(rng.integers(30, 400))
                pos = int(rng.integers(0, L - 10))
                p = [[.7, .1, .1, .1], [.1, .1, .1, .7]][k] if pos % 1000 < 500 else [.25] * 4
                seq = "".join(rng.choice(list(BASES), size=n, p=p))
                cigar = [(0, n)] if i % 7 else [(0, n // 2), (2, 3), (0, n - n // 2)]
                recs.append(synth.SynthRecord("r%d_%d" % (tid, i), tid, pos, 16 * (i % 2), cigar, n, seq=seq))
        recs.sort(key=lambda r: (r.tid, r.pos))
        path = str(d / ("sample_%s.bam" % "ab"[k]))
        synth.write_bam(path, NAMES, lengths, recs)
        names, lens, batch, _ = bm.kept_reads(path)
        assert list(lens) == lengths
        out.append((path, batch))
    return out, lengths


CMP_VARIANTS = {
    "whole": ([], dict(), 0, False),
    "whole_loose": (["--min-depth", "3", "--min-count", "1", "--min-frac", "0.2"],
                    dict(min_depth=3, min_count=1, min_ppm=200000), 0, False),
    "by100": (["--by", "100", "--min-depth", "0", "--min-count", "0", "--min-frac", "0"],
              dict(min_depth=0, min_count=0, min_ppm=0), 100, False),
    "regions_whole": (["-rc", "RC", "--min-depth", "2"], dict(min_depth=2), 0, True),
    "regions_by100": (["-rc", "RC", "--by", "100"], dict(), 100, True),
}
CLI_DEFAULTS = dict(min_depth=5, min_count=2, min_ppm=50000)


@pytest.mark.parametrize("variant", sorted(CMP_VARIANTS))
def test_cli(two_bams, tmp_path, variant):
    from metacov_amd.cli import main
    (sa, sb), lengths = two_bams
    args, kw, window, with_regions = CMP_VARIANTS[variant]
    kw = dict(CLI_DEFAULTS, **kw)
    names = NAMES
    if with_regions:
        regs = [(1, 5, 700), (0, 0, lengths[0]), (1, lengths[1] - 20, lengths[1] + 15), (1, 5, 700)]
        rc = tmp_path / "r.csv"
        rc.write_text("sequence_id,start,stop\n" + "".join("%s,%d,%d\n" % (names[t], x, z) for t, x, z in regs))
    else:
        regs = [(t, 0, L) for t, L in enumerate(lengths)]
    tids, starts, ends = (np.array(x, np.int64) for x in zip(*regs))
    seg_off, pa = bm.counts_model(sa[1], tids, starts, ends)
    _, pb = bm.counts_model(sb[1], tids, starts, ends)
    first, rows = cm.compare_model(pa, pb, seg_off, window, **kw)
    want = cm.tsv([names[t] for t, _, _ in regs], [x for _, x, _ in regs], seg_off, window, first, rows)
    args = [str(tmp_path / "r.csv") if x == "RC" else x for x in args]
    texts = []
    for decode in ("host", "gpu"):
        out = tmp_path / ("%s.tsv" % decode)
        r = CliRunner().invoke(main, ["compare", "-b", sa[0], "-c", sb[0], "-o", str(out), "--decode", decode] + args)
        assert r.exit_code == 0, r.output
        texts.append(out.read_text())
    assert texts[0] == texts[1]
    assert texts[0] == want
    assert rows[:, cm.COMPARED].sum() > 0 and rows[:, cm.CON_DIFF].sum() > 0 and rows[:, cm.DIST_FIX].sum() > 0
    # and the writer over the model gives these bytes
    fh = io.StringIO()
    mb.write_compare(fh, [names[t] for t, _, _ in regs], [x for _, x, _ in regs], mb.Comparison(first, rows, window))
    assert fh.getvalue() == want


def test_compare_convenience(two_bams):
    (sa, sb), lengths = two_bams
    x, z = 10, lengths[1] // 2
    tids, starts, ends = np.array([1]), np.array([x]), np.array([z])
    seg_off, pa = bm.counts_model(sa[1], tids, starts, ends)
    _, pb = bm.counts_model(sb[1], tids, starts, ends)
    first, rows = cm.compare_model(pa, pb, seg_off, 64, min_depth=3)
    for decode in ("host", "gpu"):
        got = mb.compare(sa[0], sb[0], "ctg_2", x, z, window=64, min_depth=3, decode=decode)
        assert np.array_equal(got.rows, rows) and np.array_equal(got.win_first, first)
    whole = mb.compare(sa[0], sb[0], "ctg_1", min_depth=3)
    assert whole.rows[0, cm.POSITIONS] == lengths[0]
    with pytest.raises(KeyError):
        mb.compare(sa[0], sb[0], "no_such_contig")
