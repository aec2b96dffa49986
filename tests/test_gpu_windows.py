"""Windowed coverage on the GPU (csrc/windows.hip) against the model in
tests/windows_model.py applied to the oracle's depth vector: exact equality
of seg_first, sum, ge and of the histogram rows.  Shapes are a few tiles; T
(tile), the smallest window, the most bins and the histogram's workgroup
count come from the library."""
import ctypes
import os

import numpy as np
import pytest

from metacov_amd import _lib
from metacov_amd import windows as mwin
from metacov_amd.bam import BamFile
from metacov_amd.engine import CoverageEngine
from oracle import coracle
from tests import runs_model, windows_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(lib_built):
    e = CoverageEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def DIMS(lib_built):
    return mwin.dims()            # (T, min_window, max_bins, hist_groups)


def load_vectors(eng, vectors, lengths=None):
    """Contig t gets depth vectors[t], built from reads of span 1 (as
    test_stats_cases does).  Returns the oracle's (depth, ext, coff)."""
    vectors = [np.asarray(v, np.int64) for v in vectors]
    lengths = [len(v) for v in vectors] if lengths is None else lengths
    pos = np.concatenate([np.repeat(np.arange(len(v)), v) for v in vectors]).astype(np.int32)
    tid = np.concatenate([np.full(int(v.sum()), t) for t, v in enumerate(vectors)]).astype(np.int32)
    return load_reads(eng, lengths, tid, pos, np.ones(len(pos), np.int32))


def load_reads(eng, lengths, tid, pos, span):
    eng.set_contigs(np.asarray(lengths, np.int64))
    eng.add_reads(tid, pos, span)
    eng.compute_depth()
    return coracle.depth(lengths, tid, pos, span)


def load_layers(eng, lengths, layers):
    """layers: (tid, pos, span, count) -> count reads each."""
    tid = np.concatenate([np.full(c, t) for t, _, _, c in layers]).astype(np.int32)
    pos = np.concatenate([np.full(c, p) for _, p, _, c in layers]).astype(np.int32)
    span = np.concatenate([np.full(c, s) for _, _, s, c in layers]).astype(np.int32)
    order = np.lexsort((pos, tid))
    return load_reads(eng, lengths, tid[order], pos[order], span[order])


def check(eng, oracle, tids, starts, ends, window, thr=None):
    d, ext, coff = oracle
    got = eng.depth_windows(tids, starts, ends, window=window, thresholds=thr)
    sf, s, ge = windows_model.windows_model(d, ext, coff, tids, starts, ends, window, thr)
    assert got.seg_first.dtype == np.int64 and got.sum.dtype == np.int64 and got.ge.dtype == np.int64
    assert np.array_equal(got.seg_first, sf)
    assert np.array_equal(got.sum, s)
    assert got.ge.shape == ge.shape and np.array_equal(got.ge, ge)
    return got


def check_hist(eng, oracle, tids, starts, ends, n_bins):
    d, ext, coff = oracle
    got = eng.depth_hist(tids, starts, ends, n_bins=n_bins)
    want = windows_model.hist_model(d, ext, coff, tids, starts, ends, n_bins)
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want)
    assert np.array_equal(got.sum(axis=1), np.maximum(0, np.asarray(ends) - np.asarray(starts)))
    return got


def whole(lengths):
    n = len(lengths)
    return np.arange(n, dtype=np.int32), np.zeros(n, np.int64), np.asarray(lengths, np.int64)


def expected_tiles(eng, tids, starts, ends, window, T):
    """The tile table's length as the header describes it: a window of at most
    T - 3 positions lies in one tile, which holds whole windows up to T - lead
    positions; a longer window is cut into pieces of at most T - lead."""
    base = eng.depth_device()[0] // 4
    n = 0
    for t, a, b in zip(tids, starts, ends):
        t, a, b = int(t), int(a), int(b)
        if b <= a:
            continue
        at = base + eng.contig_offset(t)[0]
        win = b - a if window == 0 or window > b - a else window
        if win <= T - 3:
            while a < b:
                a += min((T - ((at + a) & 3)) // win * win, b - a)
                n += 1
        else:
            for wa in range(a, b, win):
                we = min(wa + win, b)
                while wa < we:
                    wa += min(T - ((at + wa) & 3), we - wa)
                    n += 1
    return n


# ------------------------------------------------------- tile and window edges

@pytest.mark.parametrize("wname", ["16", "17", "100", "T-1", "T", "T+1", "3T+5", "0"])
def test_tile_and_window_edges(eng, DIMS, wname):
    """One contig of each length 1, T-1, T, T+1, 2T+1 (contig offsets are odd,
    leads non-zero), a depth step at position T, every window size around the
    tile: the short last window, a window longer than its segment."""
    T = DIMS[0]
    window = {"16": 16, "17": 17, "100": 100, "T-1": T - 1, "T": T, "T+1": T + 1, "3T+5": 3 * T + 5, "0": 0}[wname]
    rng = np.random.default_rng(3)
    vecs = []
    for n in (1, T - 1, T, T + 1, 2 * T + 1):
        v = rng.integers(0, 3, size=n)
        v[T:] += 2
        vecs.append(v)
    o = load_vectors(eng, vecs)
    lens = [len(v) for v in vecs]
    got = check(eng, o, *whole(lens), window, [1, 2, 3])
    want_rows = [1 if window == 0 else -(-n // window) for n in lens]
    assert np.diff(got.seg_first).tolist() == want_rows
    assert got.length().sum() == sum(lens)
    assert eng._windows.timing()["tiles"] == expected_tiles(eng, *whole(lens), window, T)
    check(eng, o, *whole(lens), window)                       # no thresholds


def test_step_at_tile_and_window_boundary(eng, DIMS):
    """Depth 1 on [0, T), 2 on [T, 2T) of a contig at offset 0: position T
    starts a tile and a window, for windows inside a tile and for whole-tile
    windows."""
    T = DIMS[0]
    v = np.ones(2 * T, np.int64)
    v[T:] = 2
    o = load_vectors(eng, [v])
    for window in (T // 8, T // 2, T, 16):
        got = check(eng, o, [0], [0], [2 * T], window, [2])
        k = T // window
        assert got.sum[:k].tolist() == [window] * k and got.sum[k:].tolist() == [2 * window] * k
        assert got.ge[:k, 0].tolist() == [0] * k and got.ge[k:, 0].tolist() == [window] * k


# ------------------------------------------------------ both regimes in a call

def test_both_regimes(eng, DIMS):
    T = DIMS[0]
    rng = np.random.default_rng(7)
    lens = [3 * T + 7, 50, T // 2, 2 * T + 100]
    vecs = [rng.integers(0, 5, size=n) for n in lens]
    o = load_vectors(eng, vecs)
    segs = whole(lens)
    got = check(eng, o, *segs, 0, [1, 4])                     # rows of 4 tiles, 1 tile, 1 tile, 3 tiles
    tiles = eng._windows.timing()["tiles"]
    assert tiles == expected_tiles(eng, *segs, 0, T) and tiles >= 4 + 1 + 1 + 3
    assert got.sum.tolist() == [int(v.sum()) for v in vecs]
    for window in (2 * T + 3, T + 1, 3 * T):                  # long windows with short last ones, and short segments
        check(eng, o, *segs, window, [1, 4])
        assert eng._windows.timing()["tiles"] == expected_tiles(eng, *segs, window, T)
    t = eng._windows.timing()
    assert t["window_ms"] > 0 and t["combine_ms"] >= 0


# ------------------------------------------------------------------ sub-ranges

@pytest.mark.parametrize("window", [0, 16, 100, "T+5"])
def test_subranges(eng, DIMS, window):
    T = DIMS[0]
    window = T + 5 if window == "T+5" else window
    rng = np.random.default_rng(5)
    L = 2 * T + 37
    v = rng.integers(0, 3, size=L)
    o = load_vectors(eng, [np.array([1, 1, 1, 2]), v])        # contig 1 starts at offset 4: aligned
    segs = [(1, 1, 50), (1, 2, T + 3), (1, 3, L), (1, 5, 6), (1, T - 1, T + 1), (1, T, T + 2),
            (1, 7, L - 5),                                    # an end inside the extent
            (1, 0, L),                                        # at the extent
            (1, 9, L + 100),                                  # past the extent
            (1, L - 1, L + 1), (1, L, L + 9), (1, L + 4, L + 2 * T),   # at / entirely past the extent
            (1, 10, 10), (1, L + 3, L + 3), (0, 0, 0),        # empty
            (1, 7, L - 5), (1, 7, L - 5),                     # duplicated
            (1, 100, T), (1, 50, 2 * T),                      # overlapping, unsorted
            (0, 1, 3), (0, 0, 5)]
    tids, starts, ends = (np.array(x) for x in zip(*segs))
    got = check(eng, o, tids, starts, ends, window, [0, 1])
    for i in (10, 11):                                        # entirely past the extent
        a, b = got.seg_first[i], got.seg_first[i + 1]
        assert b > a and not got.sum[a:b].any() and not got.ge[a:b, 1].any()
        assert np.array_equal(got.ge[a:b, 0], got.length()[a:b])      # a threshold of 0: the window length
    for i in (12, 13, 14):
        assert got.seg_first[i] == got.seg_first[i + 1]
    assert np.array_equal(got.ge[:, 0], got.length())
    check_hist(eng, o, tids, starts, ends, 3)


def test_many_segments(eng, DIMS):
    """More segments than histogram workgroups, on tiny tiles."""
    T, _, _, G = DIMS
    rng = np.random.default_rng(11)
    lens = [T + 1, 300, 2 * T - 3, 5, 64]
    o = load_vectors(eng, [rng.integers(0, 4, size=n) for n in lens])
    k = G + 37
    tids = rng.integers(0, len(lens), size=k).astype(np.int32)
    starts = np.array([rng.integers(0, lens[t] + 2) for t in tids], np.int64)
    ends = starts + rng.integers(0, 40, size=k)
    check(eng, o, tids, starts, ends, 0, [1, 2])
    check(eng, o, tids, starts, ends, 16, [1, 2])
    check_hist(eng, o, tids, starts, ends, 5)


# ------------------------------------------------- segments far past the extent

def test_segments_at_2_31_and_2_40(eng, DIMS):
    """Segments around 2^31 and ending at 2^40 (the largest end the calls
    accept), about 3 T positions each, beside one inside the extent: sums,
    threshold counts and histogram all zero there, the window bounds exact
    in 64 bits, for windows that do not divide the segments."""
    T = DIMS[0]
    rng = np.random.default_rng(17)
    L = T + 9
    v = rng.integers(1, 4, size=L)
    o = load_vectors(eng, [np.array([1, 2, 1]), v])
    far = [(1, 2 ** 31 - 5, 2 ** 31 + T + 5), (1, 2 ** 40 - 3 * T - 7, 2 ** 40), (0, 2 ** 31 - 5, 2 ** 31 + T + 5),
           (1, 2 ** 31 - 1, 2 ** 31), (1, 2 ** 31, 2 ** 31 + 1), (1, 2 ** 40 - 1, 2 ** 40)]
    segs = far[:2] + [(1, 5, L + 3)] + far[2:]
    tids, starts, ends = (np.array(x, np.int64) for x in zip(*segs))
    assert ends.max() == 2 ** 40 and (ends - starts).max() <= 3 * T + 7
    is_far = np.array([s != segs[2] for s in segs])
    for window in (0, 16, 100, 1000, T + 5):
        assert window == 0 or any((int(b) - int(a)) % window for _, a, b in far[:3])
        got = check(eng, o, tids, starts, ends, window, [0, 1, 3])
        seg, ws, we = windows_model.window_bounds(starts, ends, window)
        assert np.array_equal(got.segment_of(), seg)
        assert np.array_equal(got.start(), ws) and np.array_equal(got.end(), we)
        f = is_far[seg]
        assert not got.sum[f].any() and not got.ge[f, 1:].any() and got.sum[~f].sum() == v[5:].sum()
        assert np.array_equal(got.ge[:, 0], we - ws)
        assert got.start().max() == 2 ** 40 - 1 and got.end().max() == 2 ** 40
    h = check_hist(eng, o, tids, starts, ends, 4)
    assert np.array_equal(h[is_far, 0], (ends - starts)[is_far]) and not h[is_far, 1:].any()


# ------------------------------------------------------------------ thresholds

@pytest.mark.parametrize("thr", [[], [3], list(range(1, 17)), [0, 4, 100, 101, 2 ** 31 - 1]])
def test_thresholds(eng, DIMS, thr):
    """Depths exactly at each threshold and one below, over more than a tile,
    in windows inside a tile, whole tiles and whole segments."""
    T = DIMS[0]
    vals = sorted({0, 1, 2, 3, 4, 5, 15, 16, 17, 99, 100, 101})
    v = np.resize(np.repeat(vals, 3), T + 11)
    o = load_vectors(eng, [v, np.array([0, 1, 1, 4, 4, 3])])
    lens = [len(v), 6]
    for window in (0, 16, 300, T + 3):
        got = check(eng, o, *whole(lens), window, thr)
        assert got.ge.shape == (len(got), len(thr))
        if thr and thr[0] == 0:
            assert np.array_equal(got.ge[:, 0], got.length()) and not got.ge[:, -1].any()
    if thr == [3]:                                             # the same through the spec string
        again = eng.depth_windows(*whole(lens), window=16, thresholds="3")
        want = eng.depth_windows(*whole(lens), window=16, thresholds=[3])
        assert np.array_equal(again.ge, want.ge) and np.array_equal(again.sum, want.sum)


# ---------------------------------------------------------------- 64-bit sums

def test_sums_beyond_int32(eng, DIMS):
    T = DIMS[0]
    n = 300_000
    o = load_reads(eng, [3 * T], np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, 3 * T, np.int32))
    got = check(eng, o, [0], [0], [3 * T], T, [n, n + 1])
    assert got.sum.tolist() == [n * T] * 3 and n * T > 2 ** 31
    assert got.ge.tolist() == [[T, 0]] * 3
    got = check(eng, o, [0], [0], [3 * T], 0, [n])
    assert got.sum.tolist() == [n * 3 * T] and got.ge.tolist() == [[3 * T]]
    check(eng, o, [0], [0], [3 * T], T - 192, [n])            # one window per tile, finished there
    h = check_hist(eng, o, [0], [0], [3 * T + 5], 8)
    assert h[0].tolist() == [5, 0, 0, 0, 0, 0, 0, 3 * T]
    # windows that share a tile: the LDS accumulators pass 2^31
    n = 600_000
    o = load_reads(eng, [3 * T], np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, 3 * T, np.int32))
    got = check(eng, o, [0], [0], [3 * T], T // 2, [n])
    assert got.sum.tolist() == [n * (T // 2)] * 6 and n * (T // 2) > 2 ** 31


# ------------------------------------------------------------------- histogram

def test_hist_bins(eng, DIMS):
    """Depths at n_bins - 2, n_bins - 1, n_bins and far above for every bin
    count, on two contigs and sub-ranges."""
    T, _, B, _ = DIMS
    L = T + 100
    layers = [(0, 100, T - 50, 15), (0, 200, 300, 1), (0, 300, 200, 1),           # 15, 16, 17
              (0, 1000, 40, B - 2 - 15), (0, 1010, 30, 1), (0, 1020, 20, 1),      # B - 2, B - 1, B
              (0, 1030, 10, 12000),                                               # far above
              (1, 1, 5, 1), (1, 2, 3, 1), (1, 3, 1, 1)]                           # 0 1 2 3 2 1 0
    o = load_layers(eng, [L, 7], layers)
    d = o[0]
    assert d[1005] == B - 2 and d[1015] == B - 1 and d[1025] == B and d[1035] == B + 12000
    segs = [(0, 0, L), (1, 0, 7), (0, 990, 1050), (0, 0, L), (0, 50, T), (1, 3, 3), (1, 5, 30), (0, L + 5, L + 9)]
    tids, starts, ends = (np.array(x) for x in zip(*segs))
    for n_bins in (1, 2, 17, B):
        h = check_hist(eng, o, tids, starts, ends, n_bins)
        assert np.array_equal(h[0], h[3])                      # duplicated: its own full row
        assert not h[5].any()                                  # empty
        assert h[7, 0] == 4 and h[7].sum() == 4                # past the extent: bin 0
        if n_bins == B:
            assert h[2, B - 2] == 10 and h[2, B - 1] == 10 + 10 + 10
        if n_bins == 17:
            assert h[0, 15] > 0 and h[0, 16] > 0
    assert eng._windows.timing()["hist_ms"] > 0


def test_hist_long_segment_and_large_combine(eng, DIMS):
    """One segment of more than 2 hist_groups tiles at constant depth 1:
    several workgroups flush into its row; the same contig as one window is
    more than 2000 partial rows for the combine pass."""
    T, _, _, G = DIMS
    L = (2 * G + 1) * T + 5
    pos = np.arange(0, L, 3 * T, dtype=np.int64)
    span = np.minimum(3 * T, L - pos)
    eng.set_contigs(np.array([L, 40], np.int64))
    eng.add_reads(np.zeros(len(pos), np.int32), pos.astype(np.int32), span.astype(np.int32))
    eng.compute_depth()
    segs = (np.array([1, 0, 0], np.int32), np.array([0, 0, 3], np.int64), np.array([40, L, L + 2], np.int64))
    h = eng.depth_hist(*segs, n_bins=4)
    assert h.tolist() == [[40, 0, 0, 0], [0, L, 0, 0], [2, L - 3, 0, 0]]
    again = eng.depth_hist(*segs, n_bins=4)
    assert np.array_equal(h, again)
    wc = eng.depth_windows(*segs, window=0, thresholds=[1, 2])
    assert wc.sum.tolist() == [0, L, L - 3] and wc.ge.tolist() == [[0, 0], [L, 0], [L - 3, 0]]
    assert eng._windows.timing()["tiles"] == expected_tiles(eng, *segs, 0, T) >= 2 * (2 * G + 1)
    wc = eng.depth_windows(*segs, window=1000 * T, thresholds=[1])
    assert wc.sum.tolist() == [0, 1000 * T, 1000 * T, L - 2000 * T, 1000 * T, 1000 * T, L - 3 - 2000 * T]
    assert np.array_equal(wc.ge[:, 0], wc.sum)


def test_hist_leaves_windows_readable(eng, DIMS):
    T = DIMS[0]
    rng = np.random.default_rng(2)
    v = rng.integers(0, 9, size=T + 500)
    o = load_vectors(eng, [v])
    h = mwin._handle(eng)
    thr = np.array([2, 5], np.int32)
    segs = (np.array([0], np.int32), np.array([3], np.int64), np.array([T + 400], np.int64))
    n, sf = h.compute(eng._h, *segs, 64, thr)
    s0, ge0 = h.get(0, n)
    check_hist(eng, o, [0, 0], [0, 100], [T + 500, 300], 6)
    s1, ge1 = h.get(0, n)
    sf1 = np.zeros(2, np.int64)
    assert _lib.load().mc_windows_seg_first(h._h, _lib.ptr(sf1)) == 0
    assert np.array_equal(s0, s1) and np.array_equal(ge0, ge1) and np.array_equal(sf, sf1)
    want = windows_model.windows_model(*o, *segs, 64, thr)
    assert np.array_equal(s1, want[1]) and np.array_equal(ge1, want[2])


# ------------------------------------------------------------ errors and state

def _raw_compute(lib, h, ctx, tids, starts, ends, window, thr):
    tids, starts, ends = np.asarray(tids, np.int32), np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    thr = np.asarray(thr, np.int32)
    n = ctypes.c_int64(-1)
    rc = lib.mc_windows_compute(h, ctx, len(tids), _lib.ptr(tids), _lib.ptr(starts), _lib.ptr(ends), window,
                                len(thr), _lib.ptr(thr), ctypes.byref(n))
    return rc, n.value


def _raw_hist(lib, h, ctx, tids, starts, ends, n_bins):
    tids, starts, ends = np.asarray(tids, np.int32), np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    out = np.full((len(tids), max(1, min(n_bins, 1 << 14))), -1, np.int64)
    rc = lib.mc_windows_hist(h, ctx, len(tids), _lib.ptr(tids), _lib.ptr(starts), _lib.ptr(ends), n_bins,
                             _lib.ptr(out))
    return rc, out


def test_errors_and_state(lib_built, DIMS):
    T, W0, B, _ = DIMS
    assert W0 == 16 and B >= 4096
    lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.check(lib.mc_windows_create(0, ctypes.byref(h)))
    INV, STATE = _lib.MC_E_INVALID, _lib.MC_E_STATE
    with CoverageEngine(0) as e:
        e.set_contigs(np.array([50, T + 9], np.int64))
        e.add_reads(np.array([0, 1, 1], np.int32), np.array([3, 0, T], np.int32), np.array([4, 2, 5], np.int32))
        assert _raw_compute(lib, h, e._h, [0], [0], [50], 0, [])[0] == STATE           # depth not computed
        assert _raw_hist(lib, h, e._h, [0], [0], [50], 4)[0] == STATE
        buf = np.zeros(4, np.int64)
        assert lib.mc_windows_seg_first(h, _lib.ptr(buf)) == STATE
        assert lib.mc_windows_get(h, 0, 0, None, None) == STATE
        f, t64 = ctypes.c_float(), ctypes.c_int64()
        assert lib.mc_windows_timing(h, ctypes.byref(f), ctypes.byref(f), ctypes.byref(f), ctypes.byref(t64)) == STATE
        e.compute_depth()
        for window in (1, 15, -1):
            assert _raw_compute(lib, h, e._h, [0], [0], [50], window, [])[0] == INV, window
        for thr in ([4, 1], [1, 1], [-1, 3], list(range(17))):
            assert _raw_compute(lib, h, e._h, [0], [0], [50], 0, thr)[0] == INV, thr
        assert _raw_compute(lib, h, e._h, [2], [0], [5], 0, [])[0] == INV               # bad tid
        assert _raw_compute(lib, h, e._h, [-1], [0], [5], 0, [])[0] == INV
        assert _raw_compute(lib, h, e._h, [0], [6], [5], 0, [])[0] == INV               # end < start
        assert _raw_compute(lib, h, e._h, [0], [0], [2 ** 40 + 1], 0, [])[0] == INV
        assert _raw_compute(lib, h, e._h, [0, 0], [0, -1], [5, 5], 0, [])[0] == INV
        assert b"segment 1" in lib.mc_last_error()
        assert lib.mc_windows_seg_first(h, _lib.ptr(buf)) == STATE                      # still nothing computed
        for n_bins in (0, -1, B + 1):
            assert _raw_hist(lib, h, e._h, [0], [0], [50], n_bins)[0] == INV, n_bins
        assert _raw_hist(lib, h, e._h, [2], [0], [50], 4)[0] == INV
        assert _raw_hist(lib, h, e._h, [0], [9], [8], 4)[0] == INV
        # contig 0: depth 1 on [3, 7); contig 1: 1 on [0, 2) and [T, T + 5)
        rc, n = _raw_compute(lib, h, e._h, [0, 1], [0, 0], [50, T + 9], 20, [1])
        n1 = (T + 9 + 19) // 20
        assert (rc, n) == (0, 3 + n1)
        s, ge = np.zeros(n, np.int64), np.zeros(n, np.int64)
        assert lib.mc_windows_get(h, 0, n, _lib.ptr(s), _lib.ptr(ge)) == 0
        assert s[:4].tolist() == [4, 0, 0, 2] and ge[:4].tolist() == [4, 0, 0, 2] and s.sum() == 4 + 2 + 5
        assert lib.mc_windows_get(h, 3, 1, _lib.ptr(s), _lib.ptr(ge)) == 0 and (s[0], ge[0]) == (2, 2)
        assert lib.mc_windows_get(h, n, 0, None, None) == 0
        assert lib.mc_windows_get(h, 0, 1, _lib.ptr(s), None) == INV                    # ge needed with a threshold
        for first, count in ((0, n + 1), (n, 1), (n + 1, 0), (-1, 1), (0, -1)):
            assert lib.mc_windows_get(h, first, count, _lib.ptr(s), _lib.ptr(ge)) == INV
        # a second compute with fewer windows exposes only the new ones; no thresholds: ge may be NULL
        rc, n = _raw_compute(lib, h, e._h, [0], [4], [30], 0, [])
        assert (rc, n) == (0, 1)
        sf = np.full(2, -1, np.int64)
        assert lib.mc_windows_seg_first(h, _lib.ptr(sf)) == 0 and sf.tolist() == [0, 1]
        assert lib.mc_windows_get(h, 0, 2, _lib.ptr(s), None) == INV
        assert lib.mc_windows_get(h, 0, 1, _lib.ptr(s), None) == 0 and s[0] == 3
        p1, p2, p3 = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        nn, nt = ctypes.c_int64(), ctypes.c_int32(-1)
        assert lib.mc_windows_device(h, ctypes.byref(p1), ctypes.byref(p2), ctypes.byref(p3), ctypes.byref(nn),
                                     ctypes.byref(nt)) == 0
        assert nn.value == 1 and nt.value == 0 and p1.value and p3.value
        # no segments at all
        assert _raw_compute(lib, h, e._h, [], [], [], 0, []) == (0, 0)
        assert _raw_compute(lib, h, e._h, [], [], [], 16, [1]) == (0, 0)
        assert lib.mc_windows_hist(h, e._h, 0, None, None, None, 4, None) == 0
        rc, out = _raw_hist(lib, h, e._h, [0, 1], [0, 0], [50, 0], 2)
        assert rc == 0 and out.tolist() == [[46, 4], [0, 0]]
        # the engine's defaults: every contig over [0, length), and the handle is reused
        wc = e.depth_windows()
        assert wc.seg_first.tolist() == [0, 1, 2] and wc.sum.tolist() == [4, 7] and wc.window == 0
        assert e.depth_windows(window=16, thresholds="1").ge[:, 0].sum() == 11
        assert e.depth_hist(n_bins=3).tolist() == [[46, 4, 0], [T + 2, 7, 0]]
        with pytest.raises(ValueError):
            e.depth_windows(starts=[0])
    assert lib.mc_windows_destroy(h) == 0


# ------------------------------------------------------------------------ fuzz

@pytest.mark.parametrize("seed", range(20))
def test_fuzz(eng, DIMS, seed):
    T, _, B, _ = DIMS
    rng = np.random.default_rng(2000 + seed)
    nc = int(rng.integers(1, 7))
    lens = rng.integers(1, 3 * T + 1, size=nc).astype(np.int64)
    n = int(rng.integers(0, 4000))
    tid = np.sort(rng.integers(0, nc, size=n)).astype(np.int32)
    pos = (rng.random(n) * lens[tid]).astype(np.int32)
    max_span = 3000 if seed % 3 == 0 else 120               # long spans: extents exceed lengths
    span = rng.integers(0, max_span, size=n).astype(np.int32)
    if seed % 3:
        span = np.minimum(span, lens[tid] - pos).astype(np.int32)
    order = np.lexsort((pos, tid))
    tid, pos, span = tid[order], pos[order], span[order]
    o = load_reads(eng, lens, tid, pos, span)
    k = int(rng.integers(1, 41))
    tids = rng.integers(0, nc, size=k).astype(np.int32)
    starts = (rng.random(k) * (lens[tids] + 20)).astype(np.int64)
    ends = starts + (rng.random(k) ** 3 * (lens[tids] + 3100)).astype(np.int64)
    window = int([0, rng.integers(16, 65), rng.integers(T - 40, T + 41), rng.integers(2 * T + 1, 3 * T),
                  rng.integers(65, T - 40)][seed % 5])
    thr = np.unique(rng.integers(0, 12, size=int(rng.integers(0, 17)))).tolist()
    n_bins = int([1, 2, rng.integers(3, 40), rng.integers(40, B + 1)][seed % 4])
    a = check(eng, o, tids, starts, ends, window, thr)
    b = eng.depth_windows(tids, starts, ends, window=window, thresholds=thr)   # two identical calls
    assert np.array_equal(a.seg_first, b.seg_first) and np.array_equal(a.sum, b.sum) and np.array_equal(a.ge, b.ge)
    ha = check_hist(eng, o, tids, starts, ends, n_bins)
    assert np.array_equal(ha, eng.depth_hist(tids, starts, ends, n_bins=n_bins))


# --------------------------------------------------------------------- goldens

@pytest.mark.parametrize("tag", ["synth_edge", "synth_multi"])
def test_goldens(eng, synth_golden, golden_dir, tag):
    g = synth_golden[tag]
    bf = BamFile(os.path.join(golden_dir, tag + ".bam"))
    eng.set_contigs(np.asarray(bf.lengths, np.int64))
    eng.add_reads(bf.tid, bf.pos, bf.span)
    eng.compute_depth()
    nc = len(bf.lengths)
    segs = (np.arange(nc), np.zeros(nc, np.int64), np.array(g["extents"], np.int64))
    r = eng.depth_runs(*segs)
    wc = eng.depth_windows(*segs, window=0, thresholds=[1])
    h = eng.depth_hist(*segs, n_bins=4)
    assert len(wc) == int((segs[2] > 0).sum())
    for t in range(nc):
        s, e, v = r.segment(t)
        vec = runs_model.expand(0, g["extents"][t], s, v).astype(np.int64)
        a, b = wc.seg_first[t], wc.seg_first[t + 1]
        if len(vec) == 0:
            assert a == b
            continue
        assert b == a + 1 and wc.sum[a] == vec.sum() and wc.ge[a, 0] == np.count_nonzero(vec)
        assert h[t].tolist() == np.bincount(np.minimum(vec, 3), minlength=4).tolist()


# -------------------------------------------------------------- CLI end to end

def _bed_lines(names, tids, starts, ends, window, thr, model):
    sf, s, ge = model
    seg, a, b = windows_model.window_bounds(starts, ends, window)
    lines = []
    if thr:
        lines.append("\t".join(["#chrom", "start", "end", "mean"] + ["%dX" % x for x in thr]))
    for i in range(len(s)):
        cols = [names[int(tids[seg[i]])], "%d" % a[i], "%d" % b[i], "%.2f" % (int(s[i]) / int(b[i] - a[i]))]
        lines.append("\t".join(cols + ["%d" % x for x in ge[i]]))
    return lines


def _dist_lines(labels, hist):
    lines = []
    for lab, row in list(zip(labels, hist)) + [("total", hist.sum(axis=0))]:
        n = int(row.sum())
        filled = [b for b in range(len(row)) if row[b]]
        for b in range(filled[-1], -1, -1) if filled else ():
            lines.append("%s\t%s\t%.4f" % (lab, "%d+" % b if b == len(row) - 1 else "%d" % b,
                                            int(row[b:].sum()) / n))
    return lines


def test_cli_coverage(golden_dir, tmp_path, lib_built):
    from click.testing import CliRunner
    from metacov_amd.cli import coverage
    bam = os.path.join(golden_dir, "synth_multi.bam")
    bf = BamFile(bam)
    names, lens = list(bf.references), list(bf.lengths)
    o = coracle.depth(lens, bf.tid, bf.pos, bf.span)
    tids, starts, ends = whole(lens)

    def run(*args):
        out = tmp_path / ("o%d.bed" % len(os.listdir(tmp_path)))
        res = CliRunner().invoke(coverage, ["-b", bam, "-o", str(out), *args])
        assert res.exit_code == 0, res.output
        return out.read_text().splitlines()

    # default: one row per contig in header order
    want = _bed_lines(names, tids, starts, ends, 0, [], windows_model.windows_model(*o, tids, starts, ends, 0, []))
    rows = run()
    assert rows == want and len(rows) == len(lens)
    assert run("--decode", "host") == want
    # fixed windows with thresholds
    model = windows_model.windows_model(*o, tids, starts, ends, 1000, [1, 4])
    assert run("--by", "1000", "--thresholds", "1,4") == _bed_lines(names, tids, starts, ends, 1000, [1, 4], model)
    # the distribution, 8 bins
    dist = tmp_path / "d.txt"
    run("--dist", str(dist), "--dist-bins", "8")
    hist = windows_model.hist_model(*o, tids, starts, ends, 8)
    assert dist.read_text().splitlines() == _dist_lines(names, hist)
    # regions, in file order, one running past its contig
    rc = tmp_path / "r.csv"
    regs = [(names[2], 100, 9000), (names[0], 0, lens[0]), (names[2], 11990, 12200), (names[5], 39000, 10)]
    rc.write_text("sequence_id,start,stop\n" + "".join("%s,%d,%d\n" % r for r in regs))
    rt = np.array([names.index(r[0]) for r in regs])
    rs = np.array([min(r[1], r[2]) for r in regs])
    re_ = np.array([max(r[1], r[2]) for r in regs])
    model = windows_model.windows_model(*o, rt, rs, re_, 500, [1])
    dist2 = tmp_path / "d2.txt"
    got = run("-rc", str(rc), "--by", "500", "--thresholds", "1", "--dist", str(dist2), "--dist-bins", "8")
    assert got == _bed_lines(names, rt, rs, re_, 500, [1], model)
    labels = ["%s:%d-%d" % (names[t], a, b) for t, a, b in zip(rt, rs, re_)]
    assert dist2.read_text().splitlines() == _dist_lines(labels, windows_model.hist_model(*o, rt, rs, re_, 8))
