"""Strand-resolved base counts without a GPU: the strand model against the
literal loop, the host source's flags against the model's BAM reader, the
writer's twelve strand columns and the CLI's option rule."""
import io
import os

import numpy as np
import pytest
from click.testing import CliRunner

from metacov_amd import _lib
from metacov_amd import bases as mb
from tests import bases_model as bm
from tests import strand_model as sm
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
        q = None if rng.random() < .2 else [int(x) for x in rng.integers(0, 41, size=k)]
        out.append((int(rng.integers(0, n_ref)), int(rng.integers(0, span)), c,
                    "".join(rng.choice(list("ACGTN"), size=k)), q))
    out.sort(key=lambda r: (r[0], r[1]))
    return out


@pytest.mark.parametrize("min_baseq", [0, 20])
def test_model_strands_sum_to_the_loop(min_baseq):
    rng = np.random.default_rng(3)
    b = bm.make_batch(_reads(rng, 120))
    flags = (rng.integers(0, 2, size=120) * 0x10 | rng.integers(0, 2, size=120) * 0x1 |
             rng.integers(0, 2, size=120) * 0x80).astype(np.uint16)
    segs = [(0, 0, 340), (1, 7, 200), (0, 100, 150)]
    tids, starts, ends = zip(*segs)
    off, total, rev = sm.counts_model(b, flags, tids, starts, ends, min_baseq)
    off2, want = bm.counts_loop(b, tids, starts, ends, min_baseq)
    assert np.array_equal(off, off2) and np.array_equal(total, want)
    assert (rev <= total).all() and 0 < rev.sum() < total.sum()
    _, total2, rev2 = sm.counts_model(b, flags, tids, starts, ends, min_baseq, loop=True)
    assert np.array_equal(total2, total) and np.array_equal(rev2, rev)
    # only bit 0x10 decides, and the split of the reads into batches does not matter
    _, _, rev3 = sm.counts_model([bm.slice_batch(b, 0, 50), bm.slice_batch(b, 50, 120)],
                                 [flags[:50] & 0x10, flags[50:] & 0x10], tids, starts, ends, min_baseq)
    assert np.array_equal(rev3, rev)
    # a deletion takes the strand of its read
    d = bm.make_batch([(0, 10, "3M2D3M", "ACGTAC", 30), (0, 11, "3M2D3M", "ACGTAC", 30)])
    _, t, r = sm.counts_model(d, [0x10, 0], [0], [0], [30])
    assert t[DEL, 13:16].tolist() == [1, 2, 1] and r[DEL, 13:16].tolist() == [1, 1, 0]


def test_sites_model_by_hand():
    #            A   C   G   T   N  DEL
    total = np.array([[9, 6, 0, 0, 0, 0],      # C passes counts; C is on the forward strand only
                      [9, 6, 0, 3, 0, 0],      # C one-stranded, T weaker but on both strands
                      [9, 6, 0, 1, 0, 0],      # the weaker T fails min_count 2
                      [9, 0, 0, 0, 0, 4],      # DEL on both strands
                      [0, 0, 0, 0, 7, 0]],     # N is no allele
                     np.int64).T
    rev = np.array([[4, 0, 0, 0, 0, 0], [4, 0, 0, 1, 0, 0], [4, 0, 0, 1, 0, 0], [4, 0, 0, 0, 0, 2],
                    [0, 0, 0, 0, 3, 0]], np.int64).T
    off = [0, 5]
    plain = bm.sites_model(total, off, [100], 1, 2, 100000)
    first, pos, cnt, rc = sm.sites_model(total, rev, off, [100], 1, 2, 100000, 0)
    assert np.array_equal(first, plain[0]) and np.array_equal(pos, plain[1]) and np.array_equal(cnt, plain[2])
    assert pos.tolist() == [100, 101, 102, 103] and np.array_equal(rc, rev.T[:4])
    first, pos, cnt, rc = sm.sites_model(total, rev, off, [100], 1, 2, 100000, 1)
    assert pos.tolist() == [101, 103] and first.tolist() == [0, 2] and rc[:, [T, DEL]].tolist() == [[1, 0], [0, 2]]
    assert sm.sites_model(total, rev, off, [100], 1, 2, 100000, 2)[1].tolist() == [103]
    assert sm.sites_model(total, rev, off, [100], 1, 2, 100000, 3)[1].tolist() == []
    # ref as a minority allele: A becomes an alternative, 5 forward and 4 reverse
    ref = np.array([1, 1, 1, 4, 4], np.uint8)
    assert sm.sites_model(total, rev, off, [100], 1, 2, 100000, 4, ref)[1].tolist() == [100, 101, 102]
    assert sm.sites_model(total, rev, off, [100], 1, 2, 100000, 5, ref)[1].tolist() == []


# ------------------------------------------------------------- the host source

@pytest.mark.parametrize("name", GOLDENS)
def test_source_flags(lib_built, golden_dir, name):
    path = os.path.join(golden_dir, name)
    want = sm.kept_flags(path)
    reads = bm.kept_reads(path)[2]
    assert len(want) == bm.n_reads(reads)
    for kw in ({}, {"max_reads": 97}, {"max_reads": 1}, {"max_bases": 1000}):
        got, n = [], 0
        with mb.BaseSource(path, 2) as src:
            assert len(src.flags()) == 0                         # no batch yet
            while True:
                b = src.next(**kw)
                if b is None:
                    break
                assert set(b) == {"tid", "pos", "cig_off", "cigar", "l_seq", "seq_off", "seq", "qual_off", "qual"}
                f = src.flags()
                assert f.dtype == np.uint16 and len(f) == len(b["tid"])
                got.append(f.copy())
                n += 1
            assert len(src.flags()) == 0                         # the end of the file: an empty batch
        assert n > 10 or not kw or name != "bbmap.sorted.bam"    # the small sizes cut the file into many batches
        assert np.array_equal(np.concatenate(got + [np.zeros(0, np.uint16)]), want), kw
    if name == "bbmap.sorted.bam":
        assert 0 < int(sm.is_reverse(want).sum()) < len(want)
        w30 = sm.kept_flags(path, flag_filter=0x714, min_mapq=30)      # 0x10 in the filter: forward reads only
        with mb.BaseSource(path, 2, flag_filter=0x714, min_mapq=30) as src:
            src.next()
            assert np.array_equal(src.flags(), w30) and len(w30) and not sm.is_reverse(w30).any()


# ------------------------------------------------------------------ the writer

def test_write_sites_strand_columns():
    assert mb.HEADER_STRAND == mb.HEADER[:-1] + ("\tA_fwd\tC_fwd\tG_fwd\tT_fwd\tN_fwd\tDEL_fwd"
                                                  "\tA_rev\tC_rev\tG_rev\tT_rev\tN_rev\tDEL_rev\n")
    fh = io.StringIO()
    n = mb.write_sites(fh, "c1", [0, 41], [[1, 2, 3, 4, 5, 6], [0, 0, 0, 0, 9, 0]],
                       rev=[[1, 0, 2, 0, 5, 3], [0, 0, 0, 0, 4, 0]])
    assert n == 2
    assert fh.getvalue() == ("c1\t1\t.\t16\t1\t2\t3\t4\t5\t6\t0\t2\t1\t4\t0\t3\t1\t0\t2\t0\t5\t3\n"
                             "c1\t42\t.\t0\t0\t0\t0\t0\t9\t0\t0\t0\t0\t0\t5\t0\t0\t0\t0\t0\t4\t0\n")
    # uint32 inputs near 2^32 do not wrap, and the first ten columns are write_sites' without rev
    big = np.array([[4000000000, 1, 0, 0, 0, 4000000000]], np.uint32)
    brev = np.array([[3999999999, 1, 0, 0, 0, 0]], np.uint32)
    a, b = io.StringIO(), io.StringIO()
    mb.write_sites(a, "c 2", [7], big, ref=np.frombuffer(b"g", np.uint8), rev=brev)
    mb.write_sites(b, "c 2", [7], big, ref=np.frombuffer(b"g", np.uint8))
    assert a.getvalue() == b.getvalue()[:-1] + "\t1\t0\t0\t0\t0\t4000000000\t3999999999\t1\t0\t0\t0\t0\n"
    fh = io.StringIO()
    assert mb.write_sites(fh, "c", [], np.zeros((0, 6)), rev=np.zeros((0, 6))) == 0 and fh.getvalue() == ""
    # the model's table agrees with the writer
    fh = io.StringIO()
    fh.write(mb.HEADER_STRAND)
    mb.write_sites(fh, "c1", [0, 2], [[1, 2, 3, 4, 5, 6], [7, 0, 0, 0, 0, 0]], ref=np.frombuffer(b"aN", np.uint8),
                   rev=[[0, 2, 1, 4, 0, 6], [3, 0, 0, 0, 0, 0]])
    assert fh.getvalue() == sm.table({0: "c1"}, [(0, 0, [1, 2, 3, 4, 5, 6], [0, 2, 1, 4, 0, 6]),
                                                 (0, 2, [7, 0, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0])], {"c1": "acN"})


# ----------------------------------------------------------------------- CLI

def test_cli_min_alt_strand_needs_strand(golden_dir):
    from metacov_amd.cli import main
    bam = os.path.join(golden_dir, "synth_exp.bam")
    r = CliRunner().invoke(main, ["bases", "-b", bam, "--min-alt-strand", "2"])
    assert r.exit_code == 2 and "--min-alt-strand needs --strand" in r.output
    r = CliRunner().invoke(main, ["bases", "-b", bam, "--strand", "--min-alt-strand", "-1"])
    assert r.exit_code == 2 and "min-alt-strand" in r.output
    r = CliRunner().invoke(main, ["bases", "--help"])
    assert r.exit_code == 0 and "--strand" in r.output and "--min-alt-strand" in r.output


def test_abi_table_has_strand():
    for name in ("mc_bases_track_strand", "mc_bases_add_batch_flags", "mc_bases_add_batch_device_flags",
                 "mc_bases_get_reverse", "mc_bases_reverse_device", "mc_bases_set_strand", "mc_bases_sites_strand",
                 "mc_bases_sites_get_reverse", "mc_bases_src_flags", "mc_bam_gpu_bases_flags",
                 "mc_bam_gpu_bases_copy_flags"):
        assert name in _lib.SIGNATURES
