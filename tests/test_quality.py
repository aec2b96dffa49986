"""Per-allele quality sums without a GPU: the event model against the literal
loop, the host source's mapq column against the model's BAM reader, the
writer's eleven quality columns and the CLI's option rules."""
import io
import os

import numpy as np
import pytest
from click.testing import CliRunner

from metacov_amd import _lib
from metacov_amd import bases as mb
from tests import bases_model as bm
from tests import quality_model as qm
from tests.bases_model import A, C, G, T, N, DEL

GOLDENS = ["bbmap.sorted.bam", "synth_edge.bam", "synth_exp.bam", "synth_exp_noseq.bam", "synth_longcigar.bam",
           "synth_multi.bam"]


# ------------------------------------------------------------------- the model

def _reads(rng, n, n_ref=2, span=300):
    cigars = ["20M", "8M2I8M", "6M3D9M", "2H4S10M", "5M7N5M", "4=2X4=", "1M", "3M1D"]
    out = []
    for _ in range(n):
        c = str(rng.choice(cigars))
        k = bm.query_length(bm.cigar_words(c))
        q = None if rng.random() < .2 else [int(x) for x in rng.integers(0, 255, size=k)]
        out.append((int(rng.integers(0, n_ref)), int(rng.integers(0, span)), c,
                    "".join(rng.choice(list("ACGTN"), size=k)), q))
    out.sort(key=lambda r: (r[0], r[1]))
    return out


@pytest.mark.parametrize("min_baseq", [0, 20])
def test_event_model_equals_the_loop(min_baseq):
    rng = np.random.default_rng(5)
    b = bm.make_batch(_reads(rng, 120))
    mapq = rng.integers(0, 256, size=120).astype(np.uint8)
    mapq[:2] = [0, 255]
    segs = [(0, 0, 340), (1, 7, 200), (0, 100, 150)]
    tids, starts, ends = zip(*segs)
    off, total, bq, mq = qm.counts_model(b, mapq, tids, starts, ends, min_baseq)
    off2, want = bm.counts_loop(b, tids, starts, ends, min_baseq)
    assert np.array_equal(off, off2) and np.array_equal(total, want)          # the counts are the plain ones
    _, total2, bq2, mq2 = qm.counts_model(b, mapq, tids, starts, ends, min_baseq, loop=True)
    assert np.array_equal(total2, total) and np.array_equal(bq2, bq) and np.array_equal(mq2, mq)
    assert bq[DEL].sum() == 0 and mq[DEL].sum() > 0 and bq.sum() > 0
    assert (bq.astype(np.int64) <= 255 * total.astype(np.int64)).all()
    assert (mq.astype(np.int64) <= 255 * total.astype(np.int64)).all()
    # the split of the reads into batches does not matter
    _, _, bq3, mq3 = qm.counts_model([bm.slice_batch(b, 0, 50), bm.slice_batch(b, 50, 120)], [mapq[:50], mapq[50:]],
                                     tids, starts, ends, min_baseq)
    assert np.array_equal(bq3, bq) and np.array_equal(mq3, mq)


def test_counts_model_by_hand():
    # a deletion adds its read's MAPQ and no quality; absent qualities count and add 0; a base below
    # min_baseq adds nothing at all
    b = bm.make_batch([(0, 10, "2M1D1M", "ACG", [30, 5, 40]), (0, 10, "3M", "AAT", None), (0, 12, "1M", "N", [254])])
    _, total, bq, mq = qm.counts_model(b, [7, 255, 0], [0], [10], [14], 10)
    #                                   pos 10          11           12            13
    assert total[A].tolist() == [2, 1, 0, 0] and total[C].tolist() == [0, 0, 0, 0] and total[T].tolist() == [0, 0, 1, 0]
    assert total[DEL].tolist() == [0, 0, 1, 0] and total[N].tolist() == [0, 0, 1, 0]
    assert total[G].tolist() == [0, 0, 0, 1]
    assert bq[A].tolist() == [30, 0, 0, 0] and mq[A].tolist() == [262, 255, 0, 0]
    assert bq[N].tolist() == [0, 0, 254, 0] and mq[N].tolist() == [0, 0, 0, 0]
    assert bq[DEL].tolist() == [0, 0, 0, 0] and mq[DEL].tolist() == [0, 0, 7, 0]
    assert bq[G].tolist() == [0, 0, 0, 40] and mq[G].tolist() == [0, 0, 0, 7] and mq[T].tolist() == [0, 0, 255, 0]


def test_sites_model_by_hand():
    #                  A   C  G  T  N DEL
    total = np.array([[9, 4, 0, 0, 0, 0],      # C: bq 80 = 20 x 4, mq 120 = 30 x 4
                      [9, 4, 0, 0, 0, 0],      # C: bq one below
                      [9, 4, 0, 0, 0, 0],      # C: mq one below
                      [9, 0, 0, 0, 0, 4],      # DEL: no quality, mq at the threshold
                      [9, 4, 0, 2, 0, 0]],     # C fails, the weaker T passes
                     np.int64).T
    bq = np.array([[300, 80, 0, 0, 0, 0], [300, 79, 0, 0, 0, 0], [300, 80, 0, 0, 0, 0], [300, 0, 0, 0, 0, 0],
                   [300, 0, 0, 40, 0, 0]], np.int64).T
    mq = np.array([[500, 120, 0, 0, 0, 0], [500, 120, 0, 0, 0, 0], [500, 119, 0, 0, 0, 0], [500, 0, 0, 0, 0, 120],
                   [500, 0, 0, 60, 0, 0]], np.int64).T
    off = [0, 5]
    plain = bm.sites_model(total, off, [100], 1, 2, 100000)
    first, pos, cnt, sb, sq = qm.sites_model(total, bq, mq, off, [100], 1, 2, 100000)
    assert np.array_equal(first, plain[0]) and np.array_equal(pos, plain[1]) and np.array_equal(cnt, plain[2])
    assert pos.tolist() == [100, 101, 102, 103, 104] and np.array_equal(sb, bq.T) and np.array_equal(sq, mq.T)
    assert qm.sites_model(total, bq, mq, off, [100], 1, 2, 100000, 20, 30)[1].tolist() == [100, 103, 104]
    assert qm.sites_model(total, bq, mq, off, [100], 1, 2, 100000, 255, 30)[1].tolist() == [103]
    assert qm.sites_model(total, bq, mq, off, [100], 1, 2, 100000, 20, 31)[1].tolist() == []
    assert qm.sites_model(total, bq, mq, off, [100], 1, 2, 100000, 21, 0)[1].tolist() == [103]
    # ref as a minority allele: A becomes the alternative there
    ref = np.array([1, 4, 4, 4, 4], np.uint8)
    assert qm.sites_model(total, bq, mq, off, [100], 1, 2, 100000, 33, 55, ref)[1].tolist() == [100]
    assert qm.sites_model(total, bq, mq, off, [100], 1, 2, 100000, 34, 55, ref)[1].tolist() == []


# ------------------------------------------------------------- the host source

def test_goldens_have_distinct_mapq(golden_dir):
    assert any(len(set(qm.kept_mapq(os.path.join(golden_dir, name)).tolist())) >= 2 for name in GOLDENS)


@pytest.mark.parametrize("name", GOLDENS)
def test_source_mapq(lib_built, golden_dir, name):
    path = os.path.join(golden_dir, name)
    want = qm.kept_mapq(path)
    assert want.dtype == np.uint8 and len(want) == bm.n_reads(bm.kept_reads(path)[2])
    for kw in ({}, {"max_reads": 97}, {"max_reads": 1}, {"max_bases": 1000}):
        got = []
        with mb.BaseSource(path, 2) as src:
            assert len(src.mapq()) == 0                          # no batch yet
            while True:
                b = src.next(**kw)
                if b is None:
                    break
                assert set(b) == {"tid", "pos", "cig_off", "cigar", "l_seq", "seq_off", "seq", "qual_off", "qual"}
                m = src.mapq()
                assert m.dtype == np.uint8 and len(m) == len(b["tid"])
                got.append(m.copy())
            assert len(src.mapq()) == 0                          # the end of the file: an empty batch
        assert np.array_equal(np.concatenate(got + [np.zeros(0, np.uint8)]), want), kw
    w30 = qm.kept_mapq(path, min_mapq=30)
    assert len(w30) <= len(want) and (w30 >= 30).all()
    got = []
    with mb.BaseSource(path, 2, min_mapq=30) as src:
        while src.next(max_reads=97) is not None:
            got.append(src.mapq().copy())
    assert np.array_equal(np.concatenate(got + [np.zeros(0, np.uint8)]), w30)


# ------------------------------------------------------------------ the writer

def test_write_sites_quality_columns():
    assert mb.HEADER_QUALITY == mb.HEADER[:-1] + ("\tA_bq\tC_bq\tG_bq\tT_bq\tN_bq"
                                                   "\tA_mq\tC_mq\tG_mq\tT_mq\tN_mq\tDEL_mq\n")
    fh = io.StringIO()
    n = mb.write_sites(fh, "c1", [0, 41], [[1, 2, 3, 4, 5, 6], [0, 0, 0, 0, 9, 0]],
                       bq=[[30, 41, 52, 63, 74, 0], [0, 0, 0, 0, 90, 0]],
                       mq=[[60, 120, 180, 240, 255, 7], [0, 0, 0, 0, 2295, 0]])
    assert n == 2
    assert fh.getvalue() == ("c1\t1\t.\t16\t1\t2\t3\t4\t5\t6\t30\t41\t52\t63\t74\t60\t120\t180\t240\t255\t7\n"
                             "c1\t42\t.\t0\t0\t0\t0\t0\t9\t0\t0\t0\t0\t0\t90\t0\t0\t0\t0\t2295\t0\n")
    # uint32 sums near 2^32 are written as they are, and the first ten columns are write_sites' without them
    cnt = np.array([[4000000000, 1, 0, 0, 0, 4000000000]], np.uint32)
    bq = np.array([[4294967295, 254, 0, 0, 0, 0]], np.uint32)
    mq = np.array([[4294967295, 255, 0, 0, 0, 4294967294]], np.uint32)
    a, b = io.StringIO(), io.StringIO()
    mb.write_sites(a, "c 2", [7], cnt, ref=np.frombuffer(b"g", np.uint8), bq=bq, mq=mq)
    mb.write_sites(b, "c 2", [7], cnt, ref=np.frombuffer(b"g", np.uint8))
    assert a.getvalue() == b.getvalue()[:-1] + "\t4294967295\t254\t0\t0\t0\t4294967295\t255\t0\t0\t0\t4294967294\n"
    fh = io.StringIO()
    assert mb.write_sites(fh, "c", [], np.zeros((0, 6)), bq=np.zeros((0, 6)), mq=np.zeros((0, 6))) == 0
    assert fh.getvalue() == ""
    with pytest.raises(ValueError, match="together"):
        mb.write_sites(io.StringIO(), "c", [1], [[1, 0, 0, 0, 0, 0]], bq=[[1, 0, 0, 0, 0, 0]])
    # the model's table agrees with the writer
    fh = io.StringIO()
    fh.write(mb.HEADER_QUALITY)
    mb.write_sites(fh, "c1", [0, 2], [[1, 2, 3, 4, 5, 6], [7, 0, 0, 0, 0, 0]], ref=np.frombuffer(b"aN", np.uint8),
                   bq=[[9, 8, 7, 6, 5, 0], [70, 0, 0, 0, 0, 0]], mq=[[1, 2, 3, 4, 5, 6], [420, 0, 0, 0, 0, 0]])
    assert fh.getvalue() == qm.table({0: "c1"}, [(0, 0, [1, 2, 3, 4, 5, 6], [9, 8, 7, 6, 5, 0], [1, 2, 3, 4, 5, 6]),
                                                 (0, 2, [7, 0, 0, 0, 0, 0], [70, 0, 0, 0, 0, 0],
                                                  [420, 0, 0, 0, 0, 0])], {"c1": "acN"})


# ----------------------------------------------------------------------- CLI

def test_cli_quality_option_errors(golden_dir):
    from metacov_amd.cli import main
    bam = os.path.join(golden_dir, "synth_exp.bam")
    r = CliRunner().invoke(main, ["bases", "-b", bam, "--min-alt-baseq", "20"])
    assert r.exit_code == 2 and "--min-alt-baseq needs --quality" in r.output
    r = CliRunner().invoke(main, ["bases", "-b", bam, "--min-alt-mapq", "20"])
    assert r.exit_code == 2 and "--min-alt-mapq needs --quality" in r.output
    r = CliRunner().invoke(main, ["bases", "-b", bam, "--quality", "--strand"])
    assert r.exit_code == 2 and "--quality and --strand" in r.output
    for opt in ("--min-alt-baseq", "--min-alt-mapq"):
        for bad in ("-1", "256"):
            r = CliRunner().invoke(main, ["bases", "-b", bam, "--quality", opt, bad])
            assert r.exit_code == 2 and opt[2:] in r.output
    r = CliRunner().invoke(main, ["bases", "--help"])
    assert r.exit_code == 0 and all(o in r.output for o in ("--quality", "--min-alt-baseq", "--min-alt-mapq"))


def test_abi_table_has_quality():
    for name in ("mc_bases_track_quality", "mc_bases_add_batch_mapq", "mc_bases_add_batch_device_mapq",
                 "mc_bases_get_quality", "mc_bases_quality_device", "mc_bases_set_quality", "mc_bases_sites_quality",
                 "mc_bases_sites_get_quality", "mc_bases_quality_dims", "mc_bases_src_mapq", "mc_bam_gpu_bases_mapq",
                 "mc_bam_gpu_bases_copy_mapq"):
        assert name in _lib.SIGNATURES
