"""Depth runs on the GPU (csrc/runs.hip) against the model in
tests/runs_model.py applied to the oracle's depth vector: exact equality of
seg_first, start and value.  Shapes are a few tiles at most; T (tile) and W
(tiles per scan iteration) come from the library."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from metacov_amd import _lib
from metacov_amd import runs as mruns
from metacov_amd.bam import BamFile
from metacov_amd.engine import CoverageEngine
from oracle import coracle
from tests import runs_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(lib_built):
    e = CoverageEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def TW(lib_built):
    return mruns.dims()


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


def check(eng, oracle, tids, starts, ends, edges=None):
    d, ext, coff = oracle
    got = eng.depth_runs(tids, starts, ends, quantize=edges)
    sf, s, v = runs_model.runs_model(d, ext, coff, tids, starts, ends, edges)
    assert got.seg_first.dtype == np.int64 and got.start.dtype == np.int64 and got.value.dtype == np.int32
    assert np.array_equal(got.seg_first, sf)
    assert np.array_equal(got.start, s)
    assert np.array_equal(got.value, v)
    return got


def whole(lengths):
    n = len(lengths)
    return np.arange(n, dtype=np.int32), np.zeros(n, np.int64), np.asarray(lengths, np.int64)


# ------------------------------------------------------ tile and segment edges

@pytest.mark.parametrize("shape", ["step_at_T", "constant"])
def test_tile_edges(eng, TW, shape):
    """One contig of each length 1, T-1, T, T+1, 2T+1 (so contig offsets are
    odd too): a depth change exactly at position T, and constant depth across
    T, which must not start a run."""
    T, _ = TW
    vecs = []
    for n in (1, T - 1, T, T + 1, 2 * T + 1):
        v = np.ones(n, np.int64)
        if shape == "step_at_T":
            v[T:] = 2
        vecs.append(v)
    o = load_vectors(eng, vecs)
    got = check(eng, o, *whole([len(v) for v in vecs]))
    per_seg = np.diff(got.seg_first).tolist()
    assert per_seg == ([1, 1, 1, 2, 2] if shape == "step_at_T" else [1, 1, 1, 1, 1])
    if shape == "step_at_T":
        assert got.segment(4)[0].tolist() == [0, T]


def test_constant_empty_and_alternating(eng, TW):
    T, _ = TW
    n_alt = 2 * T + 3
    vecs = [np.full(3 * T, 3), np.zeros(T + 5, np.int64), 1 + (np.arange(n_alt) % 2)]
    o = load_vectors(eng, vecs)
    got = check(eng, o, *whole([len(v) for v in vecs]))
    assert np.diff(got.seg_first).tolist() == [1, 1, n_alt]        # one run, one zero run, a run per position
    assert got.segment(1)[2].tolist() == [0]
    assert np.array_equal(got.segment(2)[0], np.arange(n_alt))
    assert np.array_equal(got.ends()[got.seg_first[2]:], np.arange(n_alt) + 1)


# ------------------------------------------------------------------ sub-ranges

@pytest.mark.parametrize("last", [0, 2])
def test_subranges(eng, TW, last):
    T, _ = TW
    rng = np.random.default_rng(5 + last)
    L = T + 37
    v = rng.integers(0, 3, size=L)
    v[L // 2:L // 2 + 40] = 1
    v[-1] = last
    v[-2] = 1
    o = load_vectors(eng, [np.array([1, 1, 1]), v])       # contig 1 starts at offset 3
    segs = [(1, 1, 50), (1, 2, T + 3), (1, 3, L), (1, 5, 6), (1, T - 1, T + 1), (1, T, T + 2),
            (1, 7, L - 5),                                # an end inside the extent
            (1, 9, L + 100),                              # past the extent: trailing zeros
            (1, L - 1, L + 1), (1, L, L + 9), (1, L + 4, L + 2 * T),   # at / past the extent: one zero run
            (1, 10, 10), (1, L + 3, L + 3), (0, 0, 0),    # empty
            (0, 1, 3), (0, 0, 5)]
    tids, starts, ends = (np.array(x) for x in zip(*segs))
    got = check(eng, o, tids, starts, ends)
    s, e, val = got.segment(7)
    assert e[-1] == L + 100 and val[-1] == 0
    assert s[-1] == (L if last else L - 1)                # a non-zero last depth adds a zero run at the extent
    for i in (9, 10):
        assert got.segment(i)[2].tolist() == [0] and got.segment(i)[0].tolist() == [starts[i]]
    for i in (11, 12, 13):
        assert got.seg_first[i] == got.seg_first[i + 1]


# --------------------------------------------------------------- multi-segment

def test_multi_segment(eng, TW):
    T, W = TW
    rng = np.random.default_rng(11)
    lens = [T + 1, 300, 2 * T - 3, 5, 64]
    vecs = [rng.integers(0, 4, size=n) for n in lens]
    for a, b in zip(vecs, vecs[1:]):
        b[0] = a[-1] = 2                                   # equal values across every contig boundary
    o = load_vectors(eng, vecs)
    order = rng.permutation(len(lens))
    tids, starts, ends = whole(lens)
    got = check(eng, o, tids[order], starts[order], ends[order])
    assert np.all(np.diff(got.seg_first) >= 1)
    got = check(eng, o, tids, starts, ends)                # adjacent contigs: runs break at the boundary
    for i in range(1, len(lens)):
        assert got.start[got.seg_first[i]] == 0 and got.value[got.seg_first[i]] == 2
    # duplicates and overlaps
    segs = [(0, 10, T), (0, 10, T), (0, 5, 2000), (2, T - 9, T + 9), (0, 1000, T + 1), (2, 0, 2 * T - 3),
            (2, T - 9, T + 9)]
    check(eng, o, *(np.array(x) for x in zip(*segs)))
    # more tiles than one scan iteration, on tiny tiles
    k = 2 * W + 3
    tids = rng.integers(0, len(lens), size=k).astype(np.int32)
    starts = np.array([rng.integers(0, lens[t] + 2) for t in tids], np.int64)
    ends = starts + rng.integers(1, 6, size=k)
    got = check(eng, o, tids, starts, ends)
    assert eng._runs.timing()["tiles"] == k


# ------------------------------------------------- segments far past the extent

def test_segments_at_2_31_and_2_40(eng, TW):
    """Segments around 2^31 and ending at 2^40 (the largest end the call
    accepts), about 3 T positions each, beside one inside the extent: one
    zero run per far segment, its start reported exactly in 64 bits."""
    T, _ = TW
    rng = np.random.default_rng(17)
    L = T + 9
    v = rng.integers(0, 3, size=L)
    v[0] = v[-1] = 1
    o = load_vectors(eng, [np.array([1, 2, 1]), v])
    far = [(1, 2 ** 31 - 5, 2 ** 31 + T + 5), (1, 2 ** 40 - 3 * T - 7, 2 ** 40), (0, 2 ** 31 - 5, 2 ** 31 + T + 5),
           (1, 2 ** 31 - 1, 2 ** 31), (1, 2 ** 31, 2 ** 31 + 1), (1, 2 ** 40 - 1, 2 ** 40)]
    segs = far[:2] + [(1, 5, L + 3)] + far[2:]
    tids, starts, ends = (np.array(x, np.int64) for x in zip(*segs))
    assert ends.max() == 2 ** 40 and (ends - starts).max() <= 3 * T + 7
    for edges, zero in ((None, 0), ([0, 2], 1), ([1, 2], 0)):
        got = check(eng, o, tids, starts, ends, edges)
        for i in (0, 1, 3, 4, 5, 6):
            s, e, val = got.segment(i)
            assert s.tolist() == [int(starts[i])] and e.tolist() == [int(ends[i])] and val.tolist() == [zero]
        assert got.seg_first[3] - got.seg_first[2] > 2 and got.segment(2)[1][-1] == L + 3
    assert got.start.max() == 2 ** 40 - 1 and got.ends().max() == 2 ** 40


# ---------------------------------------------------------------- quantisation

@pytest.mark.parametrize("edges", [[1], [1, 4, 100], list(range(1, 17)), [3, 2 ** 31 - 1]])
def test_quantise(eng, TW, edges):
    T, _ = TW
    # depths exactly on every small edge and one below it, over more than a tile
    vals = sorted({0, 1, 2, 3, 4, 5, 15, 16, 17, 99, 100, 101})
    v = np.resize(np.repeat(vals, 3), T + 11)
    v[T - 1], v[T] = 3, 4                                  # classes meet at the tile boundary
    o = load_vectors(eng, [v, np.array([0, 1, 1, 4, 4, 3])])
    lens = [len(v), 6]
    got = check(eng, o, *whole(lens), edges=edges)
    assert got.value.max() <= len(edges)
    check(eng, o, np.array([0, 0, 1]), np.array([1, T - 2, 2]), np.array([T + 2, T + 40, 30]), edges=edges)
    # the same through the spec string
    if edges == [1, 4, 100]:
        again = eng.depth_runs(*whole(lens), quantize="0:1:4:100:")
        assert np.array_equal(again.start, got.start) and np.array_equal(again.value, got.value)


# ------------------------------------------------------------ errors and state

def _raw_compute(lib, h, ctx, tids, starts, ends, edges):
    tids, starts, ends = np.asarray(tids, np.int32), np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    edges = np.asarray(edges, np.int32)
    n = ctypes.c_int64(-1)
    rc = lib.mc_runs_compute(h, ctx, len(tids), _lib.ptr(tids), _lib.ptr(starts), _lib.ptr(ends), len(edges),
                             _lib.ptr(edges), ctypes.byref(n))
    return rc, n.value


def test_errors_and_state(lib_built, TW):
    T, _ = TW
    lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.check(lib.mc_runs_create(0, ctypes.byref(h)))
    with CoverageEngine(0) as e:
        e.set_contigs(np.array([50, T + 9], np.int64))
        e.add_reads(np.array([0, 1, 1], np.int32), np.array([3, 0, T], np.int32), np.array([4, 2, 5], np.int32))
        assert _raw_compute(lib, h, e._h, [0], [0], [50], [])[0] == _lib.MC_E_STATE      # depth not computed
        buf = np.zeros(4, np.int64)
        assert lib.mc_runs_seg_first(h, _lib.ptr(buf)) == _lib.MC_E_STATE
        e.compute_depth()
        for edges in ([4, 1], [1, 1], [-1, 3], list(range(17))):
            assert _raw_compute(lib, h, e._h, [0], [0], [50], edges)[0] == _lib.MC_E_INVALID, edges
        assert _raw_compute(lib, h, e._h, [2], [0], [5], [])[0] == _lib.MC_E_INVALID     # bad tid
        assert _raw_compute(lib, h, e._h, [-1], [0], [5], [])[0] == _lib.MC_E_INVALID
        assert _raw_compute(lib, h, e._h, [0], [6], [5], [])[0] == _lib.MC_E_INVALID     # end < start
        assert _raw_compute(lib, h, e._h, [0], [-1], [5], [])[0] == _lib.MC_E_INVALID
        assert b"segment 0" in lib.mc_last_error()
        # [0,3) 0 | [3,7) 1 | [7,50) 0 ; contig 1: [0,2) 1 | [2,T) 0 | [T,T+5) 1 | [T+5,T+9) 0
        rc, n = _raw_compute(lib, h, e._h, [0, 1], [0, 0], [50, T + 9], [])
        assert (rc, n) == (0, 7)
        s, v = np.zeros(7, np.int64), np.zeros(7, np.int32)
        assert lib.mc_runs_get(h, 0, 7, _lib.ptr(s), _lib.ptr(v)) == 0
        assert s.tolist() == [0, 3, 7, 0, 2, T, T + 5] and v.tolist() == [0, 1, 0, 1, 0, 1, 0]
        assert lib.mc_runs_get(h, 5, 2, _lib.ptr(s), _lib.ptr(v)) == 0 and s[:2].tolist() == [T, T + 5]
        assert lib.mc_runs_get(h, 7, 0, None, None) == 0
        for first, count in ((0, 8), (7, 1), (8, 0), (-1, 1), (0, -1)):
            assert lib.mc_runs_get(h, first, count, _lib.ptr(s), _lib.ptr(v)) == _lib.MC_E_INVALID
        # a second compute with fewer runs returns only the new ones
        rc, n = _raw_compute(lib, h, e._h, [0], [4], [6], [])
        assert (rc, n) == (0, 1)
        sf = np.full(2, -1, np.int64)
        assert lib.mc_runs_seg_first(h, _lib.ptr(sf)) == 0 and sf.tolist() == [0, 1]
        assert lib.mc_runs_get(h, 0, 2, _lib.ptr(s), _lib.ptr(v)) == _lib.MC_E_INVALID
        assert lib.mc_runs_get(h, 0, 1, _lib.ptr(s), _lib.ptr(v)) == 0 and (s[0], v[0]) == (4, 1)
        p1, p2, p3, nn = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
        assert lib.mc_runs_device(h, ctypes.byref(p1), ctypes.byref(p2), ctypes.byref(p3), ctypes.byref(nn)) == 0
        assert nn.value == 1 and p1.value and p2.value and p3.value
        # no segments at all
        assert _raw_compute(lib, h, e._h, [], [], [], []) == (0, 0)
        # the engine's default: every contig over [0, length), and the handle is reused
        r = e.depth_runs()
        assert r.seg_first.tolist() == [0, 3, 7] and e.depth_runs().start.tolist() == r.start.tolist()
    assert lib.mc_runs_destroy(h) == 0


# ------------------------------------------------------------------------ fuzz

@pytest.mark.parametrize("seed", range(20))
def test_fuzz(eng, TW, seed):
    T, _ = TW
    rng = np.random.default_rng(1000 + seed)
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
    edges = None
    if seed % 2:
        edges = np.unique(rng.integers(0, 12, size=int(rng.integers(1, 17)))).tolist()
    a = check(eng, o, tids, starts, ends, edges)
    b = eng.depth_runs(tids, starts, ends, quantize=edges)  # two identical calls, identical arrays
    assert np.array_equal(a.seg_first, b.seg_first) and np.array_equal(a.start, b.start)
    assert np.array_equal(a.value, b.value)


# --------------------------------------------------------------------- goldens

@pytest.mark.parametrize("tag", ["synth_edge", "synth_multi"])
def test_goldens(eng, synth_golden, golden_dir, tag):
    g = synth_golden[tag]
    bf = BamFile(os.path.join(golden_dir, tag + ".bam"))
    eng.set_contigs(np.asarray(bf.lengths, np.int64))
    eng.add_reads(bf.tid, bf.pos, bf.span)
    eng.compute_depth()
    nc = len(bf.lengths)
    r = eng.depth_runs(np.arange(nc), np.zeros(nc, np.int64), np.array(g["extents"], np.int64))
    for t in range(nc):
        s, e, v = r.segment(t)
        vec = np.ascontiguousarray(runs_model.expand(0, g["extents"][t], s, v), dtype="<i4")
        assert len(vec) == g["extents"][t]
        assert hashlib.sha256(vec.tobytes()).hexdigest() == g["depth_sha"][t]
        assert not np.any(v[1:] == v[:-1])


# -------------------------------------------------------------- CLI end to end

def _parse_bedgraph(path):
    rows = []
    with open(path) as fh:
        for line in fh:
            name, a, b, v = line.rstrip("\n").split("\t")
            rows.append((name, int(a), int(b), v))
    return rows


def test_cli_depth(golden_dir, tmp_path, lib_built):
    from click.testing import CliRunner
    from metacov_amd.cli import depth as cli_depth
    bam = os.path.join(golden_dir, "synth_multi.bam")
    bf = BamFile(bam)
    names, lens = list(bf.references), list(bf.lengths)
    d, ext, coff = coracle.depth(lens, bf.tid, bf.pos, bf.span)

    def run(*args):
        out = tmp_path / ("o%d.bedgraph" % len(os.listdir(tmp_path)))
        res = CliRunner().invoke(cli_depth, ["-b", bam, "-o", str(out), *args])
        assert res.exit_code == 0, res.output
        return _parse_bedgraph(out)

    rows = run()
    # tiles [0, length) of every contig in header order, no two adjacent equal values
    at = 0
    for t, (name, n) in enumerate(zip(names, lens)):
        mine = []
        while at < len(rows) and rows[at][0] == name:
            mine.append(rows[at])
            at += 1
        assert mine and mine[0][1] == 0 and mine[-1][2] == n, name
        assert all(a[2] == b[1] and a[3] != b[3] for a, b in zip(mine, mine[1:]))
        assert all(a < b for _, a, b, _ in mine)
        vec = np.concatenate([np.full(b - a, int(v)) for _, a, b, v in mine])
        assert np.array_equal(vec, d[coff[t]:coff[t] + n]), name
    assert at == len(rows)
    # --no-zero: the same lines minus the zero ones
    assert run("--no-zero") == [r for r in rows if r[3] != "0"]
    # --quantize: the model's classes, as labels
    labels = ["0:1", "1:4", "4:inf"]
    tids, starts, ends = np.arange(len(lens)), np.zeros(len(lens), np.int64), np.array(lens, np.int64)
    sf, s, v = runs_model.runs_model(d, ext, coff, tids, starts, ends, [1, 4])
    want = []
    for t in range(len(lens)):
        ss, vv = s[sf[t]:sf[t + 1]], v[sf[t]:sf[t + 1]]
        ee = np.append(ss[1:], lens[t])
        want += [(names[t], int(a), int(b), labels[c]) for a, b, c in zip(ss, ee, vv)]
    assert run("--quantize", "0:1:4:") == want
    assert run("--quantize", "0:1:4:", "--no-zero", "--decode", "host") == [w for w in want if w[3] != "0:1"]
    # regions, in file order, one running past its contig
    rc = tmp_path / "r.csv"
    regs = [(names[2], 100, 9000), (names[0], 0, lens[0]), (names[2], 11990, 12200), (names[5], 39000, 10)]
    rc.write_text("sequence_id,start,stop\n" + "".join("%s,%d,%d\n" % r for r in regs))
    rt = np.array([names.index(r[0]) for r in regs])
    rs = np.array([min(r[1], r[2]) for r in regs])
    re_ = np.array([max(r[1], r[2]) for r in regs])
    sf, s, v = runs_model.runs_model(d, ext, coff, rt, rs, re_)
    want = []
    for i in range(len(regs)):
        ss, vv = s[sf[i]:sf[i + 1]], v[sf[i]:sf[i + 1]]
        ee = np.append(ss[1:], re_[i])
        want += [(regs[i][0], int(a), int(b), str(c)) for a, b, c in zip(ss, ee, vv)]
    assert run("-rc", str(rc)) == want
