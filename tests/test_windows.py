"""Windowed coverage, host side: the test model against a naive loop, the
thresholds grammar, the two writers, WindowCoverage's arithmetic, the
`coverage` command's options and the ABI table.  No GPU."""
import io
import os

import numpy as np
import pytest
from click.testing import CliRunner

from metacov_amd import _lib
from metacov_amd import windows as mwin
from tests import windows_model


# ------------------------------------------------------------------ model

def _random_case(rng):
    nc = int(rng.integers(1, 5))
    ext = rng.integers(1, 90, size=nc).astype(np.int64)
    coff = np.zeros(nc + 1, np.int64)
    coff[1:] = np.cumsum(ext)
    depth = rng.integers(0, 6, size=int(coff[-1])).astype(np.int32)
    for _ in range(3):
        a = int(rng.integers(0, len(depth)))
        depth[a:a + int(rng.integers(1, 30))] = rng.integers(0, 5)
    k = int(rng.integers(1, 12))
    tids = rng.integers(0, nc, size=k).astype(np.int32)
    starts = np.array([rng.integers(0, ext[t] + 6) for t in tids], np.int64)
    ends = starts + rng.integers(0, 80, size=k)             # past the extent, and empty ones
    ends[rng.integers(0, k)] = starts[rng.integers(0, k)] if k > 1 else ends[0]
    ends = np.maximum(ends, starts)
    return depth, ext, coff[:-1], tids, starts, ends


@pytest.mark.parametrize("seed", range(30))
def test_model_matches_loop(seed):
    rng = np.random.default_rng(seed)
    depth, ext, coff, tids, starts, ends = _random_case(rng)
    window = [0, 16, 17, 1000][seed % 4]                    # 1000: larger than any segment
    thr = [None, [1], [0, 2, 5], [3, 4]][(seed // 4) % 4]   # thresholds on exact depth values
    a = windows_model.windows_model(depth, ext, coff, tids, starts, ends, window, thr)
    b = windows_model.windows_loop(depth, ext, coff, tids, starts, ends, window, thr)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)
    for n_bins in (1, 2, 4, 9):
        h = windows_model.hist_model(depth, ext, coff, tids, starts, ends, n_bins)
        assert np.array_equal(h, windows_model.hist_loop(depth, ext, coff, tids, starts, ends, n_bins))
        assert np.array_equal(h.sum(axis=1), ends - starts)


def test_model_far_past_the_extent():
    """Segments around 2^31 and ending at 2^40 (the GPU test's): the models
    against the loops, zero sums there, the window bounds exact."""
    rng = np.random.default_rng(3)
    depth, ext, coff, _, _, _ = _random_case(rng)
    segs = [(0, 2 ** 31 - 5, 2 ** 31 + 70), (0, 2 ** 40 - 200, 2 ** 40), (0, 0, int(ext[0]) + 3), (0, 2 ** 31 - 1, 2 ** 31),
            (0, 2 ** 40 - 1, 2 ** 40)]
    tids, starts, ends = (np.array(x, np.int64) for x in zip(*segs))
    for window in (0, 16, 17, 1000):
        a = windows_model.windows_model(depth, ext, coff, tids, starts, ends, window, [0, 1])
        b = windows_model.windows_loop(depth, ext, coff, tids, starts, ends, window, [0, 1])
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)
        seg, ws, we = windows_model.window_bounds(starts, ends, window)
        assert np.array_equal(a[2][:, 0], we - ws) and not a[1][seg != 2].any() and not a[2][seg != 2, 1].any()
        assert ws.max() == 2 ** 40 - 1 and we.max() == 2 ** 40 and len(ws) == len(a[1])
    h = windows_model.hist_model(depth, ext, coff, tids, starts, ends, 4)
    assert np.array_equal(h, windows_model.hist_loop(depth, ext, coff, tids, starts, ends, 4))
    assert np.array_equal(h[[0, 1, 3, 4], 0], (ends - starts)[[0, 1, 3, 4]])


def test_model_by_hand():
    depth = np.array([0, 0, 2, 2, 5, 0, 7, 7], np.int32)      # contig 0: [0,5) ; contig 1: [5,8)
    ext, coff = np.array([5, 3]), np.array([0, 5])
    sf, s, ge = windows_model.windows_model(depth, ext, coff, [0, 1, 0, 1], [0, 0, 3, 1], [7, 3, 3, 40], 0, [0, 2, 6])
    assert sf.tolist() == [0, 1, 2, 2, 3]
    assert s.tolist() == [9, 14, 14]
    assert ge.tolist() == [[7, 3, 0], [3, 2, 2], [39, 2, 2]]
    sf, s, ge = windows_model.windows_model(depth, ext, coff, [1], [1], [40], 16, [7])
    assert sf.tolist() == [0, 3] and s.tolist() == [14, 0, 0] and ge.tolist() == [[2], [0], [0]]
    seg, a, b = windows_model.window_bounds([1], [40], 16)
    assert (seg.tolist(), a.tolist(), b.tolist()) == ([0, 0, 0], [1, 17, 33], [17, 33, 40])
    h = windows_model.hist_model(depth, ext, coff, [0, 1, 0], [0, 0, 2], [7, 3, 2], 3)
    assert h.tolist() == [[4, 0, 3], [1, 0, 2], [0, 0, 0]]
    assert windows_model.hist_model(depth, ext, coff, [0], [0], [7], 1).tolist() == [[7]]


# ------------------------------------------------------------- thresholds

def test_parse_thresholds_good():
    assert mwin.parse_thresholds("1,10,30") == [1, 10, 30]
    assert mwin.parse_thresholds("0") == [0]
    assert mwin.parse_thresholds(" 1, 4 ") == [1, 4]
    assert mwin.parse_thresholds("") == []
    assert mwin.parse_thresholds(",".join(str(i) for i in range(16))) == list(range(16))
    assert mwin.parse_thresholds("3,2147483647") == [3, 2 ** 31 - 1]


@pytest.mark.parametrize("spec", ["1,1", "4,1", "-1,3", "1,,3", "a", "1.5", "1:4", "1,2147483648",
                                  ",".join(str(i) for i in range(17)), "1,"])
def test_parse_thresholds_bad(spec):
    with pytest.raises(ValueError) as e:
        mwin.parse_thresholds(spec)
    assert repr(spec) in str(e.value)


def test_parse_thresholds_not_a_string():
    with pytest.raises(ValueError):
        mwin.parse_thresholds([1, 2])


# ---------------------------------------------------------------- writers

def _wc(window=0, thr=()):
    # segments: c0 [0, 40), c1 [5, 5) (empty), c0 [10, 13)
    tids, starts, ends = [0, 1, 0], [0, 5, 10], [40, 5, 13]
    seg, a, b = windows_model.window_bounds(starts, ends, window)
    n = len(seg)
    sf = np.searchsorted(seg, np.arange(4))
    total = np.arange(n) * 7 + 1
    ge = np.arange(n * len(thr)).reshape(n, len(thr))
    return mwin.WindowCoverage(tids, starts, ends, window, list(thr), sf, total, ge)


def test_window_coverage_arithmetic():
    wc = _wc(16)
    assert wc.seg_first.tolist() == [0, 3, 3, 4] and len(wc) == 4 and wc.n_segments == 3
    assert wc.start().tolist() == [0, 16, 32, 10]
    assert wc.end().tolist() == [16, 32, 40, 13]
    assert wc.length().tolist() == [16, 16, 8, 3]
    assert wc.mean().dtype == np.float64
    assert np.array_equal(wc.mean(), np.array([1, 8, 15, 22]) / np.array([16, 16, 8, 3]))
    wc = _wc(0)
    assert wc.start().tolist() == [0, 10] and wc.end().tolist() == [40, 13]
    assert wc.sum.dtype == np.int64 and wc.ge.dtype == np.int64 and wc.ge.shape == (2, 0)
    with pytest.raises(ValueError):
        mwin.WindowCoverage([0], [0], [5], 0, [], [0, 2], [1], np.zeros((1, 0)))


def test_write_windows_bed_bytes():
    out = io.StringIO()
    assert mwin.write_windows_bed(_wc(16), ["chrA", "chrB"], out) == 4
    assert out.getvalue() == ("chrA\t0\t16\t0.06\n"
                              "chrA\t16\t32\t0.50\n"
                              "chrA\t32\t40\t1.88\n"
                              "chrA\t10\t13\t7.33\n")
    out = io.StringIO()
    assert mwin.write_windows_bed(_wc(0, (1, 10)), ["chrA", "chrB"], out) == 2
    assert out.getvalue() == ("#chrom\tstart\tend\tmean\t1X\t10X\n"
                              "chrA\t0\t40\t0.03\t0\t1\n"
                              "chrA\t10\t13\t2.67\t2\t3\n")
    out = io.StringIO()                                     # a later part of one file: no header
    mwin.write_windows_bed(_wc(0, (1, 10)), ["chrA", "chrB"], out, header=False)
    assert out.getvalue() == "chrA\t0\t40\t0.03\t0\t1\nchrA\t10\t13\t2.67\t2\t3\n"
    out = io.StringIO()                                     # nothing to write: the header alone
    empty = mwin.WindowCoverage([], [], [], 0, [5], [0], [], [])
    assert mwin.write_windows_bed(empty, [], out) == 0 and out.getvalue() == "#chrom\tstart\tend\tmean\t5X\n"
    # sums beyond 2^53 / 2^31 keep their integer columns exact
    big = mwin.WindowCoverage([0], [0], [4], 0, [0], [0, 1], [2 ** 40], [[4]])
    out = io.StringIO()
    mwin.write_windows_bed(big, ["c"], out)
    assert out.getvalue().splitlines()[1] == "c\t0\t4\t%.2f\t4" % (2 ** 38)


def test_write_dist_bytes():
    hist = np.array([[2, 0, 1, 1],       # a: 4 positions, depths 0 0 2 and one >= 3
                     [0, 0, 0, 0],       # b: length 0, writes nothing
                     [3, 1, 0, 0]])      # c: highest non-empty bin 1
    out = io.StringIO()
    n = mwin.write_dist(hist, ["a", "b", "c"], out)
    assert out.getvalue() == ("a\t3+\t0.2500\n"
                              "a\t2\t0.5000\n"
                              "a\t1\t0.5000\n"
                              "a\t0\t1.0000\n"
                              "c\t1\t0.2500\n"
                              "c\t0\t1.0000\n"
                              "total\t3+\t0.1250\n"
                              "total\t2\t0.2500\n"
                              "total\t1\t0.3750\n"
                              "total\t0\t1.0000\n")
    assert n == 10
    out = io.StringIO()                  # one bin: everything is "0+"
    mwin.write_dist(np.array([[5]]), ["x"], out)
    assert out.getvalue() == "x\t0+\t1.0000\ntotal\t0+\t1.0000\n"
    out = io.StringIO()                  # no rows, or only empty ones: nothing, not even a total
    assert mwin.write_dist(np.zeros((0, 4), np.int64), [], out) == 0
    assert mwin.write_dist(np.zeros((1, 4), np.int64), ["e"], out) == 0 and out.getvalue() == ""


# -------------------------------------------------------------------- CLI

GOLDEN_BAM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synth_multi.bam")


@pytest.mark.parametrize("args, hint", [(["--by", "1"], "--by"), (["--by", "15"], "--by"), (["--by", "-1"], "--by"),
                                        (["--thresholds", "10,1"], "--thresholds"),
                                        (["--thresholds", "x"], "--thresholds"),
                                        (["--dist-bins", "0"], "--dist-bins")])
def test_cli_bad_options(args, hint):
    from metacov_amd.cli import coverage
    res = CliRunner().invoke(coverage, ["-b", GOLDEN_BAM, *args])
    assert res.exit_code == 2 and hint in res.output, res.output


def test_cli_refuses_world_size(monkeypatch):
    from metacov_amd.cli import coverage
    monkeypatch.setenv("WORLD_SIZE", "2")
    res = CliRunner().invoke(coverage, ["-b", GOLDEN_BAM])
    assert res.exit_code == 2 and "one process" in res.output


def test_cli_depth_and_pileup_still_there():
    from metacov_amd.cli import main
    assert {"pileup", "depth", "coverage"} <= set(main.commands)


# -------------------------------------------------------------------- ABI

def test_signatures_cover_the_windows_section():
    names = {"mc_windows_create", "mc_windows_destroy", "mc_windows_compute", "mc_windows_seg_first",
             "mc_windows_get", "mc_windows_device", "mc_windows_hist", "mc_windows_timing", "mc_windows_dims"}
    assert names <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["mc_windows_compute"]) == 10 and len(_lib.SIGNATURES["mc_windows_hist"]) == 8
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "metacov_amd.h")).read()
    assert "#define MC_WINDOWS_MIN 16" in header and mwin.MIN_WINDOW == 16
