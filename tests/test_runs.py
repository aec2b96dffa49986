"""Depth runs, host side: the test model against a naive loop, the quantize
grammar, the bedGraph writer, the `depth` command's options and the ABI
table.  No GPU."""
import io
import os

import numpy as np
import pytest
from click.testing import CliRunner

from metacov_amd import _lib
from metacov_amd import runs as mruns
from tests import runs_model


# ------------------------------------------------------------------ model

def _random_case(rng):
    nc = int(rng.integers(1, 5))
    ext = rng.integers(1, 60, size=nc).astype(np.int64)
    coff = np.zeros(nc + 1, np.int64)
    coff[1:] = np.cumsum(ext)
    depth = rng.integers(0, 4, size=int(coff[-1])).astype(np.int32)
    # long constant stretches as well as noise
    for _ in range(3):
        a = int(rng.integers(0, len(depth)))
        depth[a:a + int(rng.integers(1, 30))] = rng.integers(0, 3)
    k = int(rng.integers(1, 12))
    tids = rng.integers(0, nc, size=k).astype(np.int32)
    starts = np.array([rng.integers(0, ext[t] + 6) for t in tids], np.int64)
    ends = starts + rng.integers(0, 50, size=k)
    return depth, ext, coff[:-1], tids, starts, ends


@pytest.mark.parametrize("seed", range(30))
def test_model_matches_loop(seed):
    rng = np.random.default_rng(seed)
    depth, ext, coff, tids, starts, ends = _random_case(rng)
    edges = [None, [1], [1, 3], [2]][seed % 4]
    a = runs_model.runs_model(depth, ext, coff, tids, starts, ends, edges)
    b = runs_model.runs_loop(depth, ext, coff, tids, starts, ends, edges)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)


def test_model_far_past_the_extent():
    """Segments around 2^31 and ending at 2^40 (the GPU test's): the model
    against the loop, one zero run each with its start exact."""
    rng = np.random.default_rng(3)
    depth, ext, coff, _, _, _ = _random_case(rng)
    segs = [(0, 2 ** 31 - 5, 2 ** 31 + 70), (0, 2 ** 40 - 200, 2 ** 40), (0, 0, int(ext[0]) + 3), (0, 2 ** 31 - 1, 2 ** 31),
            (0, 2 ** 40 - 1, 2 ** 40)]
    tids, starts, ends = (np.array(x, np.int64) for x in zip(*segs))
    for edges in (None, [0, 2], [1]):
        a = runs_model.runs_model(depth, ext, coff, tids, starts, ends, edges)
        b = runs_model.runs_loop(depth, ext, coff, tids, starts, ends, edges)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and np.array_equal(x, y)
        sf, start, value = a
        for i in (0, 1, 3, 4):
            assert start[sf[i]:sf[i + 1]].tolist() == [segs[i][1]]
            assert value[sf[i]:sf[i + 1]].tolist() == [1 if edges == [0, 2] else 0]


def test_model_by_hand():
    depth = np.array([0, 0, 2, 2, 5, 0, 7, 7], np.int32)      # contig 0: [0,5) ; contig 1: [5,8)
    ext, coff = np.array([5, 3]), np.array([0, 5])
    sf, s, v = runs_model.runs_model(depth, ext, coff, [0, 1, 0, 1], [0, 0, 3, 4], [7, 3, 3, 6])
    assert sf.tolist() == [0, 4, 6, 6, 7]
    assert s.tolist() == [0, 2, 4, 5, 0, 1, 4]
    assert v.tolist() == [0, 2, 5, 0, 0, 7, 0]
    # quantised 0:1:4: -> classes 0, 1, 2
    sf, s, v = runs_model.runs_model(depth, ext, coff, [0], [0], [7], [1, 4])
    assert (sf.tolist(), s.tolist(), v.tolist()) == ([0, 4], [0, 2, 4, 5], [0, 1, 2, 0])
    assert np.array_equal(runs_model.expand(0, 7, s, v), [0, 0, 1, 1, 2, 0, 0])


# --------------------------------------------------------------- quantize

def test_parse_quantize_good():
    assert mruns.parse_quantize("0:1:4:100:") == ([1, 4, 100], ["0:1", "1:4", "4:100", "100:inf"])
    assert mruns.parse_quantize("0:1:") == ([1], ["0:1", "1:inf"])
    assert mruns.parse_quantize("0:1:4") == ([1, 4], ["0:1", "1:4", None])
    spec = ":".join(str(i) for i in range(17)) + ":"
    edges, labels = mruns.parse_quantize(spec)
    assert edges == list(range(1, 17)) and len(labels) == 17 and labels[-1] == "16:inf"
    assert mruns.parse_quantize("0:2147483647:")[0] == [2 ** 31 - 1]


@pytest.mark.parametrize("spec", ["", ":", "0", "0:", "1:4:", "0:4:4:", "0:5:4:", "0:a:", "0::4", "0:-1:",
                                  "0:1.5:", "0:2147483648:", ":".join(str(i) for i in range(18)) + ":"])
def test_parse_quantize_bad(spec):
    with pytest.raises(ValueError):
        mruns.parse_quantize(spec)


def test_quantise_is_searchsorted_right():
    d = np.array([0, 1, 3, 4, 99, 100, 101])
    assert runs_model.quantise(d, [1, 4, 100]).tolist() == [0, 1, 1, 2, 2, 3, 3]
    assert runs_model.quantise(d, None).tolist() == d.tolist()


# --------------------------------------------------------------- bedGraph

def _hand_runs():
    # segment 0: contig 1 [0, 10): 0 x3, 5 x4, 0 x3 ; segment 1: empty ; segment 2: contig 0 [2, 6): 7 x4
    return mruns.DepthRuns(tids=[1, 0, 0], starts=[0, 4, 2], ends=[10, 4, 6], seg_first=[0, 3, 3, 4],
                           start=[0, 3, 7, 2], value=[0, 5, 0, 7])


def test_depthruns_ends_and_segments():
    r = _hand_runs()
    assert len(r) == 4 and r.n_segments == 3
    assert r.ends().tolist() == [3, 7, 10, 6]
    s, e, v = r.segment(0)
    assert (s.tolist(), e.tolist(), v.tolist()) == ([0, 3, 7], [3, 7, 10], [0, 5, 0])
    assert [len(x) for x in r.segment(1)] == [0, 0, 0]
    s, e, v = r.segment(2)
    assert (s.tolist(), e.tolist(), v.tolist()) == ([2], [6], [7])


def test_write_bedgraph_bytes():
    r = _hand_runs()
    names = ["chrA", "chrB"]
    fh = io.StringIO()
    assert mruns.write_bedgraph(r, names, fh) == 4
    assert fh.getvalue() == "chrB\t0\t3\t0\nchrB\t3\t7\t5\nchrB\t7\t10\t0\nchrA\t2\t6\t7\n"
    fh = io.StringIO()
    assert mruns.write_bedgraph(r, names, fh, zero=False) == 2
    assert fh.getvalue() == "chrB\t3\t7\t5\nchrA\t2\t6\t7\n"


def test_write_bedgraph_labels():
    names = ["c"]
    edges, labels = mruns.parse_quantize("0:1:4:")
    r = mruns.DepthRuns([0], [0], [9], [0, 3], [0, 2, 5], [0, 2, 1], edges)
    fh = io.StringIO()
    mruns.write_bedgraph(r, names, fh, labels=labels)
    assert fh.getvalue() == "c\t0\t2\t0:1\nc\t2\t5\t4:inf\nc\t5\t9\t1:4\n"
    fh = io.StringIO()
    mruns.write_bedgraph(r, names, fh, zero=False, labels=labels)
    assert fh.getvalue() == "c\t2\t5\t4:inf\nc\t5\t9\t1:4\n"
    # a closed last class: depths at or above the last bound are left out
    _, closed = mruns.parse_quantize("0:1:4")
    fh = io.StringIO()
    assert mruns.write_bedgraph(r, names, fh, labels=closed) == 2
    assert fh.getvalue() == "c\t0\t2\t0:1\nc\t5\t9\t1:4\n"


def test_write_bedgraph_empty():
    r = mruns.DepthRuns([0], [5], [5], [0, 0], [], [])
    fh = io.StringIO()
    assert mruns.write_bedgraph(r, ["c"], fh) == 0 and fh.getvalue() == ""
    assert r.ends().tolist() == []


def test_depth_groups():
    from metacov_amd.cli import depth_groups
    assert list(depth_groups([0, 0, 0, 0], [4, 4, 4, 4], limit=8)) == [(0, 2), (2, 4)]
    assert list(depth_groups([0, 0, 0], [3, 20, 3], limit=8)) == [(0, 1), (1, 2), (2, 3)]
    assert list(depth_groups([0, 0, 0], [3, 3, 20], limit=8)) == [(0, 2), (2, 3)]
    assert list(depth_groups([], [], limit=8)) == []
    assert list(depth_groups([0], [0], limit=8)) == [(0, 1)]


# -------------------------------------------------------------------- CLI

def test_depth_help():
    from metacov_amd.cli import main
    res = CliRunner().invoke(main, ["depth", "--help"])
    assert res.exit_code == 0, res.output
    for word in ("--bamfile", "--outfile", "--regionfile-csv", "--regionfile-blast7", "--quantize",
                 "--no-zero", "--device", "--decode", "--legacy-endpos", "exact", "bedGraph"):
        assert word in res.output, word
    assert "depth" in CliRunner().invoke(main, ["--help"]).output


def test_depth_option_errors(tmp_path, golden_dir, monkeypatch):
    from metacov_amd.cli import main
    bam = os.path.join(golden_dir, "synth_multi.bam")
    run = CliRunner().invoke
    res = run(main, ["depth"])
    assert res.exit_code == 2 and "--bamfile" in res.output
    res = run(main, ["depth", "-b", str(tmp_path / "missing.bam")])
    assert res.exit_code == 2
    res = run(main, ["depth", "-b", bam, "--quantize", "1:4:"])
    assert res.exit_code == 2 and "first bound must be 0" in res.output
    res = run(main, ["depth", "-b", bam, "--decode", "pysam"])
    assert res.exit_code == 2
    rc = tmp_path / "r.csv"
    rc.write_text("sequence_id,start,stop\n")
    b7 = tmp_path / "r.blast7"
    b7.write_text("# BLASTN\n")
    res = run(main, ["depth", "-b", bam, "-rc", str(rc), "-rb", str(b7)])
    assert res.exit_code == 2 and "Only one of" in res.output
    monkeypatch.setenv("WORLD_SIZE", "2")
    res = run(main, ["depth", "-b", bam])
    assert res.exit_code == 2 and "one process" in res.output


# -------------------------------------------------------------------- ABI

def test_runs_symbols_bound():
    names = {"mc_runs_create", "mc_runs_destroy", "mc_runs_compute", "mc_runs_seg_first", "mc_runs_get",
             "mc_runs_device", "mc_runs_timing", "mc_runs_dims"}
    assert names <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["mc_runs_compute"]) == 9


def test_runs_dims_without_gpu(lib_built):
    tile, width = mruns.dims()
    assert tile >= 1024 and tile % 256 == 0 and width >= 64
