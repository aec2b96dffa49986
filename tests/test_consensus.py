"""Consensus calling without a GPU: the model in tests/consensus_model.py
against a literal loop and against cases worked out by hand, the FASTA and
summary writers' bytes, and the command's option errors."""
import io
import os

import numpy as np
import pytest
from click.testing import CliRunner

from metacov_amd import _lib
from tests import consensus_model as cm


# -------------------------------------------------------------------- model

@pytest.mark.parametrize("seed", range(6))
def test_model_matches_loop(seed):
    rng = np.random.default_rng(seed)
    n = 400
    planes = rng.integers(0, 6, size=(6, n)).astype(np.uint32)
    planes[:, rng.random(n) < 0.2] = 0
    big = rng.random(n) < 0.3                       # counts up to 2^32 - 1 in all five channels at once
    planes[:, big] = rng.integers(cm.M32 - 3, cm.M32 + 1, size=(6, int(big.sum()))).astype(np.uint32)
    planes[:, :4] = cm.M32
    ref = rng.integers(0, 6, size=n).astype(np.uint8)
    for kw in (dict(), dict(iupac=True), dict(min_depth=3, min_count=2, call_ppm=300000, iupac=True, fill_ref=True),
               dict(min_depth=int(rng.integers(0, 12)), min_count=int(rng.integers(0, 5)),
                    call_ppm=int(rng.integers(0, 1000001)), iupac=bool(seed & 1), fill_ref=bool(seed & 2)),
               dict(call_ppm=200000), dict(call_ppm=200001, iupac=True), dict(min_count=cm.M32, min_depth=5 * cm.M32)):
        for r in (None, ref):
            if r is None and kw.get("fill_ref"):
                continue
            got = cm.call(planes, ref=r, **kw)
            want = cm.call_loop(planes, ref=r, **kw)
            for g, w in zip(got, want):
                assert np.array_equal(g, w), kw


def test_model_at_the_int32_edge(lib_built):
    """The planes of bases_model.int32_edge_case (the GPU tests' read set
    around 2^31 and below 2^32): the model against the loop, and the
    segments' rows against the letters."""
    from metacov_amd import bases as mb
    from tests import bases_model as bm
    reads, segs, scrambled, k = bm.int32_edge_case(mb.dims())
    b = bm.make_batch(reads)
    for sg in (segs, scrambled):
        tids, starts, ends = (np.array(x, np.int64) for x in zip(*sg))
        off, planes = bm.counts_model(b, tids, starts, ends)
        for kw in (dict(), dict(min_depth=2, iupac=True, call_ppm=200000)):
            for g, w in zip(cm.call(planes, **kw), cm.call_loop(planes, **kw)):
                assert np.array_equal(g, w), kw
            first, summary, aligned, compact = cm.consensus_model(planes, off, **kw)
            assert np.array_equal(summary[:, 0], ends - starts) and first[-1] == len(compact)
            assert np.array_equal(aligned, cm.call(planes, **kw)[0])
            for s in range(len(sg)):
                a = aligned[off[s]:off[s + 1]]
                assert np.array_equal(compact[first[s]:first[s + 1]], a[a != ord("-")])
                assert (a != ord("N")).any(), sg[s]                         # every segment has called letters


def test_model_by_hand():
    assert len(cm.HAND) > 70
    seen = set()
    for kw, planes, ref, letters, classes, differs in cm.hand_groups():
        for fn in (cm.call, cm.call_loop):
            got_l, got_c, got_d = fn(planes, ref=ref, **kw)
            assert bytes(got_l).decode() == letters, (kw, fn.__name__)
            assert got_c.tolist() == classes and got_d.tolist() == differs, (kw, fn.__name__)
        seen |= set(classes)
    assert seen == {cm.LOW, cm.DELETED, cm.NOCALL, cm.CALLED, cm.AMBIG}
    # the 15 subsets carry the IUPAC alphabet
    iupac = {c[3] for c in cm.HAND if c[2] == {"iupac": True}}
    assert set("ACGTMRWSYKVHDBN") <= iupac


def test_model_segments():
    #                  A  C  G  T  N DEL
    cols = np.array([(3, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 2), (0, 0, 0, 0, 0, 0), (2, 2, 0, 0, 0, 0),
                     (0, 0, 0, 0, 0, 1), (0, 1, 0, 0, 0, 0)], np.uint32).T
    ref = np.array([1, 1, 1, 1, 4, 1], np.uint8)
    first, summary, aligned, compact = cm.consensus_model(cols, [0, 2, 2, 6], iupac=True, ref=ref)
    assert bytes(aligned) == b"A-NM-C" and bytes(compact) == b"ANMC"
    assert first.tolist() == [0, 1, 1, 4]
    assert summary.tolist() == [[2, 1, 0, 0, 0, 1, 2, 1], [0] * 8, [4, 1, 1, 0, 1, 1, 0, 3]]


# ------------------------------------------------------------------ writers

def test_write_fasta_bytes():
    from metacov_amd import bases as mb

    def text(name, s, **kw):
        fh = io.StringIO()
        mb.write_fasta(fh, name, np.frombuffer(s.encode(), np.uint8), **kw)
        return fh.getvalue()

    assert text("c1", "ACGTACGTAC", width=4) == ">c1\nACGT\nACGT\nAC\n"            # wrap, short last line
    assert text("c1", "ACGTACGT", width=4) == ">c1\nACGT\nACGT\n"                  # an exact multiple
    assert text("c1", "ACGT", width=4) == ">c1\nACGT\n"
    assert text("c1", "ACG", width=4) == ">c1\nACG\n"
    assert text("c 2:1-9", "ACGTN-acgt", width=0) == ">c 2:1-9\nACGTN-acgt\n"      # no wrap
    assert text("c1", "", width=4) == ">c1\n" and text("c1", "", width=0) == ">c1\n"
    s = "ACGTN" * 37
    assert text("x", s) == cm.fasta("x", np.frombuffer(s.encode(), np.uint8), 60)  # the default width
    assert text("x", s).split("\n")[1:5] == [s[0:60], s[60:120], s[120:180], s[180:]]
    for w in (0, 1, 5, 61, 184, 185, 186):
        assert text("x", s, width=w) == cm.fasta("x", np.frombuffer(s.encode(), np.uint8), w)


def test_write_summary_bytes():
    from metacov_amd import bases as mb
    fh = io.StringIO()
    rows = np.array([[10, 5, 1, 1, 2, 1, 3, 9], [0] * 8], np.int64)
    assert mb.write_consensus_summary(fh, ["c1", "c 2"], [0, 7], [10, 7], rows) == 2
    assert fh.getvalue() == ("contig\tstart\tend\tpositions\tcalled\tambiguous\tnocall\tlow\tdeleted\tdiffers\t"
                             "length\nc1\t0\t10\t10\t5\t1\t1\t2\t1\t3\t9\nc 2\t7\t7\t0\t0\t0\t0\t0\t0\t0\t0\n")
    assert fh.getvalue() == cm.summary_table([("c1", 0, 10, rows[0]), ("c 2", 7, 7, rows[1])])
    fh = io.StringIO()
    assert mb.write_consensus_summary(fh, [], [], [], np.zeros((0, 8)), header=False) == 0 and fh.getvalue() == ""
    assert mb.SUMMARY_COLUMNS[mb.DIFFERS] == "differs" and mb.SUMMARY_COLUMNS[mb.LENGTH] == "length"
    assert (mb.POSITIONS, mb.CALLED, mb.AMBIGUOUS, mb.NOCALL, mb.LOW, mb.DELETED) == (0, 1, 2, 3, 4, 5)


# ---------------------------------------------------------------------- CLI

@pytest.mark.parametrize("args, match", [
    (["--fill-ref"], "fill-ref"),
    (["--call-frac", "1.5"], "call-frac"),
    (["--call-frac", "-0.1"], "call-frac"),
    (["--call-frac", "nan"], "call-frac"),
    (["-rb", "BLAST7", "-rc", "CSV"], "Only one of"),
    (["--min-depth", "-1"], "min-depth"),
    (["--min-count", "-1"], "min-count"),
    (["--line-width", "-1"], "line-width"),
])
def test_cli_option_errors(golden_dir, tmp_path, args, match):
    from metacov_amd.cli import main
    for name in ("BLAST7", "CSV"):
        (tmp_path / name).write_text("")
    args = [str(tmp_path / a) if a in ("BLAST7", "CSV") else a for a in args]
    r = CliRunner().invoke(main, ["consensus", "-b", os.path.join(golden_dir, "synth_exp.bam")] + args)
    assert r.exit_code == 2 and match in r.output


def test_cli_world_size_and_help(golden_dir, monkeypatch):
    from metacov_amd.cli import main
    monkeypatch.setenv("WORLD_SIZE", "2")
    r = CliRunner().invoke(main, ["consensus", "-b", os.path.join(golden_dir, "synth_exp.bam")])
    assert r.exit_code == 2 and "one process" in r.output
    r = CliRunner().invoke(main, ["consensus", "--help"])
    assert r.exit_code == 0 and "never contains inserted bases" in " ".join(r.output.split())
    for opt in ("--iupac", "--fill-ref", "--aligned", "--summary", "--line-width", "--call-frac", "--decode"):
        assert opt in r.output


def test_abi_table_has_consensus():
    for name in ("mc_bases_consensus", "mc_bases_consensus_first", "mc_bases_consensus_summary",
                 "mc_bases_consensus_get", "mc_bases_consensus_device", "mc_bases_consensus_timing", "mc_bases_set"):
        assert name in _lib.SIGNATURES
