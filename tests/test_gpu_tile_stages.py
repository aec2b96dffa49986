"""What the tile stages (csrc/runs.hip, windows.hip, bases.hip) share, seen
from outside: the same verdict on a bad segment list from every entry point
that takes one, one awkward segment list through every stage against the
stages' numpy models, and the order of the in-tile compaction.  Tile sizes
come from the library."""
import ctypes
import re

import numpy as np
import pytest

from metacov_amd import _lib
from metacov_amd import bases as mb
from metacov_amd import runs as mruns
from metacov_amd import windows as mwin
from metacov_amd.engine import CoverageEngine
from tests import bases_model as bm
from tests import test_gpu_bases as tbases
from tests import test_gpu_consensus as tcons
from tests import test_gpu_diversity as tdiv
from tests import test_gpu_runs as truns
from tests import test_gpu_windows as twin

pytestmark = pytest.mark.gpu

N_REF = 3


@pytest.fixture(scope="module")
def eng(lib_built):
    e = CoverageEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def bc(lib_built):
    h = mb.BaseCounter(N_REF, 0)
    yield h
    h.close()


# ------------------------------------------------------- segment errors agree

BAD_SEGMENTS = {"tid -1": (-1, 0, 5), "tid = contigs": (N_REF, 0, 5), "start -1": (0, -1, 5),
                "end < start": (0, 6, 5), "end = 2^40 + 1": (0, 0, 2 ** 40 + 1)}


@pytest.mark.parametrize("bad", sorted(BAD_SEGMENTS) + ["null array"])
def test_segment_errors_agree(eng, bc, bad):
    """The four entry points that take a segment list return the same code and
    the same text for the same bad list (the bad segment second of three), up
    to the handle's own name."""
    lib = _lib.load()
    eng.set_contigs(np.array([101, 98, 103], np.int64))
    eng.add_reads(np.array([0, 1, 2], np.int32), np.array([3, 0, 7], np.int32), np.array([4, 2, 5], np.int32))
    eng.compute_depth()
    if bad == "null array":
        keep = (np.zeros(1, np.int64), np.ones(1, np.int64))     # (the arrays outlive the calls)
        S, tid, start, end = 1, None, _lib.ptr(keep[0]), _lib.ptr(keep[1])
    else:
        segs = [(0, 0, 50), BAD_SEGMENTS[bad], (2, 0, 50)]
        keep = (np.array([s[0] for s in segs], np.int32), np.array([s[1] for s in segs], np.int64),
                np.array([s[2] for s in segs], np.int64))
        S, (tid, start, end) = 3, (_lib.ptr(a) for a in keep)
    runs, wins = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(lib.mc_runs_create(0, ctypes.byref(runs)))
    _lib.check(lib.mc_windows_create(0, ctypes.byref(wins)))
    n, hist = ctypes.c_int64(-1), np.zeros((3, 4), np.int64)
    calls = {
        "runs": lambda: lib.mc_runs_compute(runs, eng._h, S, tid, start, end, 0, None, ctypes.byref(n)),
        "windows": lambda: lib.mc_windows_compute(wins, eng._h, S, tid, start, end, 0, 0, None, ctypes.byref(n)),
        "hist": lambda: lib.mc_windows_hist(wins, eng._h, S, tid, start, end, 4, _lib.ptr(hist)),
        "bases": lambda: lib.mc_bases_begin(bc._h, S, tid, start, end, 0),
    }
    try:
        got = {}
        for name, call in calls.items():
            rc = call()
            text = lib.mc_last_error().decode()
            got[name] = (rc, re.sub(r"the (runs|windows) handle", "the handle", text))
    finally:
        lib.mc_runs_destroy(runs)
        lib.mc_windows_destroy(wins)
    assert got["runs"][0] == _lib.MC_E_INVALID, got
    assert got["runs"][1].startswith("bad segment arrays" if bad == "null array" else "segment 1: "), got
    assert got["windows"] == got["runs"] and got["hist"] == got["runs"] and got["bases"] == got["runs"], got
    assert len(keep) in (2, 3)


# ------------------------------------- one awkward segment list, every stage

def awkward_segments(T, lead_at, room):
    """Six segments in this order: empty, one position, exactly one tile minus
    its lead, one tile plus one, that one again, one that overlaps it.  T: the
    stage's tile; lead_at(tid, start): elements of the aligned window in front
    of a tile that starts there; room[tid]: the contig's length.  The starts of
    the four distinct non-empty segments are moved by up to 3 so that their
    leads are 0, 1, 2 and 3."""
    def start_with(tid, start, lead):
        return start + ((lead - lead_at(tid, start)) & 3)

    a1 = start_with(1, 7, 3)
    a2 = start_with(2, 12, 1)
    a3 = start_with(0, 20, 2)
    a5 = start_with(0, a3 + T // 2, 0)
    segs = [(1, 5, 5), (1, a1, a1 + 1), (2, a2, a2 + T - 1), (0, a3, a3 + T + 1), (0, a3, a3 + T + 1),
            (0, a5, a5 + 300)]
    assert all(0 <= a <= b <= room[t] for t, a, b in segs)
    assert sorted({lead_at(t, a) for t, a, b in segs if b > a}) == [0, 1, 2, 3]
    return tuple(np.array(x) for x in zip(*segs))


def test_awkward_segments_depth_stages(eng):
    """Runs, windows (0 and 16) and the histogram over the list, each against
    its model; contig lengths congruent to 1, 2 and 3 mod 4."""
    T = mruns.dims()[0]
    TW = mwin.dims()[0]
    rng = np.random.default_rng(41)
    room = [max(T, TW) + 41 + 700, max(T, TW) + 102, max(T, TW) + 203]
    assert [L % 4 for L in room] == [1, 2, 3]
    vecs = [rng.integers(0, 3, size=L) for L in room]
    for v in vecs:
        v[len(v) // 3:len(v) // 3 + 50] = 1                  # a long run, and steps at both tile sizes
        v[T - 2:T + 2] = [2, 0, 1, 1]
    o = truns.load_vectors(eng, vecs)
    base = eng.depth_device()[0] // 4

    def lead_at(tid, start):
        return (base + eng.contig_offset(tid)[0] + start) & 3

    tids, starts, ends = awkward_segments(T, lead_at, room)
    got = truns.check(eng, o, tids, starts, ends)
    assert np.diff(got.seg_first)[0] == 0 and np.diff(got.seg_first)[1] == 1
    assert np.array_equal(got.segment(3)[0], got.segment(4)[0])
    truns.check(eng, o, tids, starts, ends, [1, 2])
    tids, starts, ends = awkward_segments(TW, lead_at, room)
    for window in (0, 16):
        got = twin.check(eng, o, tids, starts, ends, window, [1, 2])
        assert np.diff(got.seg_first)[0] == 0
    twin.check_hist(eng, o, tids, starts, ends, 4)


def test_awkward_segments_base_stages(bc):
    """Sites, the consensus (aligned and compact) and the diversity rows
    (windows 0 and 16) over the list on installed planes."""
    P = mb.dims()
    rng = np.random.default_rng(42)
    room = [2 * P + 41, P + 102, P + 203]
    # a bases tile leads by its plane index: the one-position segment puts the third segment at lead 1
    segs = [(1, 5, 5), (1, 7, 8), (2, 12, 12 + P - 1), (0, 20, 20 + P + 1), (0, 20, 20 + P + 1),
            (0, 20 + P // 2, 20 + P // 2 + 300)]
    assert all(0 <= a <= b <= room[t] for t, a, b in segs)
    n = sum(b - a for _, a, b in segs)
    planes = tdiv.random_planes(rng, n)
    ref = rng.integers(0, 5, size=n).astype(np.uint8)
    off = tcons.begin(bc, segs, planes)
    assert off.tolist() == np.concatenate([[0], np.cumsum([b - a for _, a, b in segs])]).tolist()
    assert [int(o) & 3 for o in off[1:6]] == [0, 1, 0, 1, 2]   # the leads of the tiles that start the segments
    assert bc.timing()["tiles"] == 1 + 1 + 2 + 2 + 1
    starts = [s[1] for s in segs]
    for r in (None, ref):
        got = tbases.check_sites(bc, planes, starts, (1, 1, 0), r)
        assert got.first[0] == got.first[1] == 0
        tbases.check_sites(bc, planes, starts, (0, 0, 0), r)
        tcons.check(bc, planes, off, ref=r)
        tcons.check(bc, planes, off, iupac=True, min_count=2, ref=r)
        for window in (0, 16):
            got = tdiv.check(bc, planes, off, window, ref=r)
            assert np.diff(got.win_first)[0] == 0


# ------------------------------------------------------------ compaction order

def edge_lanes(P):
    """Lanes 0 and 63 of every wave in every round of a bases tile."""
    k = np.arange(P)
    return np.flatnonzero((k % 64 == 0) | (k % 64 == 63))


def test_compaction_order_sites(bc):
    """Sites at lanes 0 and 63 of every (round, wave) pair of one tile, and
    nowhere else: the emit's ranks across waves and rounds."""
    P = mb.dims()
    at = edge_lanes(P)
    planes = np.zeros((6, P), np.uint32)
    planes[bm.A] = 5
    planes[bm.C, at] = 1 + np.arange(len(at))                # each site's counts name its position
    tcons.begin(bc, [(0, 100, 100 + P)], planes)
    assert bc.timing()["tiles"] == 1
    got = tbases.check_sites(bc, planes, [100], (1, 1, 0))
    assert got.pos.tolist() == (100 + at).tolist()
    assert got.counts[:, bm.C].tolist() == (1 + np.arange(len(at))).tolist()


def test_compaction_order_consensus(bc):
    """Kept letters at lanes 0 and 63 of every (round, wave) pair of one tile,
    deletions everywhere else."""
    P = mb.dims()
    at = edge_lanes(P)
    planes = np.zeros((6, P), np.uint32)
    planes[bm.DEL] = 9
    planes[bm.DEL, at] = 0
    planes[np.arange(len(at)) % 4, at] = 5                   # A C G T in turn: the order shows in the letters
    off = tcons.begin(bc, [(0, 100, 100 + P)], planes)
    got = tcons.check(bc, planes, off)
    assert got.n == len(at)
    assert bc.consensus_letters(True, 0, got.n).tobytes() == (b"ACGT" * len(at))[:len(at)]
