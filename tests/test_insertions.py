"""The insertion-allele contract (include/metacov_amd.h, "Insertion alleles")
on the CPU: the model in tests/insertions_model.py against a literal per-read
loop and against counts worked out by hand, the consensus-with-insertions
rule, the writers' bytes and the commands' option errors.  No GPU."""
import io
import os

import numpy as np
import pytest
from click.testing import CliRunner

from metacov_amd import _lib
from tests import bases_model as bm
from tests import consensus_model as cm
from tests import insertions_model as im

E = im.encode


def table(reads, segs):
    tids, starts, ends = zip(*segs)
    return im.table_rows(im.table_model(bm.make_batch(reads), tids, starts, ends))


# ------------------------------------------------------------ model and loop

@pytest.mark.parametrize("seed", range(6))
def test_model_matches_loop(seed):
    rng = np.random.default_rng(500 + seed)
    b = bm.make_batch(im.random_reads(rng, 300, n_ref=2, length=400, ins_frac=0.4), seq_gap=seed % 3)
    segs = [(0, 0, 400), (1, 50, 300), (0, 100, 200), (0, 100, 200), (1, 0, 0)]
    tids, starts, ends = zip(*segs)
    got, want = im.table_model(b, tids, starts, ends), im.table_loop(b, tids, starts, ends)
    assert len(got["i"]) > 20 and got["other"].any() and (got["count"] > 1).any()
    assert im.table_rows(got) == im.table_rows(want)
    rows = im.table_rows(got)
    keys = [(i, o, n, c) for i, n, c, o, _ in rows]
    assert keys == sorted(set(keys))                                   # sorted and unique


def test_model_at_the_int32_edge(lib_built):
    """bases_model.int32_edge_case (the GPU tests' read set): the table model
    against the literal walk, with anchors at 2^31 - 2, 2^31 - 1, 2^31, on
    both sides of a tile edge and below 2^32; the consensus with them."""
    from metacov_amd import bases as mb
    P = mb.dims()
    H = 1 << 31
    reads, segs, scrambled, k = bm.int32_edge_case(P)
    b = bm.make_batch(reads)
    for sg in (segs, scrambled):
        tids, starts, ends = (np.array(x, np.int64) for x in zip(*sg))
        got, want = im.table_model(b, tids, starts, ends), im.table_loop(b, tids, starts, ends)
        assert im.table_rows(got) == im.table_rows(want) and (got["count"] > 1).any()
        two = im.table_model([bm.slice_batch(b, 0, k), bm.slice_batch(b, k, bm.n_reads(b))], tids, starts, ends)
        assert im.table_rows(two) == im.table_rows(got)
        off, planes = bm.counts_model(b, tids, starts, ends)
        a, far, one = sg.index(segs[0]), sg.index(segs[1]), sg.index(segs[2])
        have = set(got["i"].tolist())
        for p in (H - 2, H - 1, H, segs[0][1] + P - 1, segs[0][1] + P, segs[0][1] + 2 * P - 1, segs[0][1] + 2 * P):
            assert int(off[a]) + p - segs[0][1] in have, p
        assert int(off[one]) in have                                       # 2^31 - 1 again, in its own segment
        assert any(off[far] <= i < off[far + 1] for i in have)            # the skip reads' insertion
        first, summary, inserted, aligned, compact = im.consensus_model(planes, off, got)
        assert inserted[a, 0] >= 7 and inserted[far, 0] == 1 and inserted[one, 0] == 1


# ------------------------------------------------------------- hand cases

SEG, HAND = im.SEG, im.HAND


@pytest.mark.parametrize("case", range(len(HAND)))
def test_counts_by_hand(case):
    reads, want = HAND[case]
    reads = sorted(reads, key=lambda r: (r[0], r[1]))
    assert table(reads, SEG) == want
    b = bm.make_batch(reads)
    assert im.table_rows(im.table_loop(b, [0], [100], [200])) == want


def test_segments_by_hand():
    """Duplicated and overlapping segments each get the event."""
    reads = [(0, 150, "2M2I2M", "AACGAA", 30)]
    segs = [(0, 100, 200), (0, 151, 152), (0, 100, 200), (0, 152, 160), (1, 100, 200), (0, 140, 152)]
    off = bm.seg_offsets([s[1] for s in segs], [s[2] for s in segs])
    assert off.tolist() == [0, 100, 101, 201, 209, 309, 321]
    t = im.table_model(bm.make_batch(reads), *zip(*segs))
    assert im.table_rows(t) == [(51, 2, E("CG"), 0, 1), (100, 2, E("CG"), 0, 1), (152, 2, E("CG"), 0, 1),
                                (320, 2, E("CG"), 0, 1)]
    assert im.first_of(t, off).tolist() == [0, 1, 2, 3, 3, 3, 4]


def test_code_ordering():
    """Numeric order of the codes of one length is lexicographic order."""
    seqs = [a + b + c for a in "TGCA" for b in "ACGT" for c in "GATC"]
    assert sorted(seqs) == sorted(seqs, key=im.encode) and len(set(map(im.encode, seqs))) == 64
    assert im.encode("A") == 0 and im.encode("T") == 3 and im.encode("CA") == 4 and im.encode("T" * 32) == 2 ** 64 - 1
    for s in ("A", "ACGT", "TTTT", "GATTACA", "ACGT" * 8):
        assert im.decode(len(s), im.encode(s)) == s


def test_thresholds_by_hand():
    planes = np.zeros((6, 4), np.uint32)
    planes[bm.A] = [6, 7, 2, 0]
    planes[bm.DEL] = [2, 1, 0, 0]
    planes[bm.N] = [9, 9, 9, 9]                                        # never part of the depth
    t = im.make_table([(0, 1, 0, 0, 3), (0, 0, 0, 1, 1), (1, 2, 5, 0, 7), (2, 1, 1, 0, 1), (3, 1, 2, 0, 4)])

    def kept(**kw):
        return [r[0:2] + r[4:] for r in im.table_rows(im.filter_table(t, planes, **kw))]

    assert len(kept(min_depth=0, min_count=1, min_ppm=0)) == 5         # (0, 1, 0): everything
    assert kept(min_depth=1) == [(0, 1, 3), (0, 0, 1), (1, 2, 7), (2, 1, 1)]     # depth 0 at index 3
    assert kept(min_depth=8) == [(0, 1, 3), (0, 0, 1), (1, 2, 7)]      # depth 8 at equality
    assert kept(min_depth=9) == []
    assert kept(min_count=3) == [(0, 1, 3), (1, 2, 7)] and kept(min_count=4) == [(1, 2, 7)]
    assert kept(min_ppm=375000) == [(0, 1, 3), (1, 2, 7), (2, 1, 1)]   # 3 of 8 = 375 000 ppm exactly
    assert kept(min_ppm=375001) == [(1, 2, 7), (2, 1, 1)]
    assert kept(min_ppm=875000, min_depth=0) == [(1, 2, 7), (3, 1, 4)]          # 7 of 8; depth 0 passes any ppm


# --------------------------------------------------------------- consensus

def _cons(planes_cols, rows, seg_off=None, **kw):
    planes = np.array(planes_cols, np.uint32).T.copy()
    seg_off = [0, planes.shape[1]] if seg_off is None else seg_off
    first, summary, inserted, aligned, compact = im.consensus_model(planes, seg_off, im.make_table(rows), **kw)
    return bytes(compact).decode(), first.tolist(), summary[:, cm.COL_LENGTH].tolist(), inserted.tolist()


def test_consensus_rule_by_hand():
    A5, C5, D5, LOW = (5, 0, 0, 0, 0, 0), (0, 5, 0, 0, 0, 0), (0, 0, 0, 0, 0, 5), (0, 0, 0, 0, 3, 0)
    # the top allele follows its letter; OTHER is never called, even with the highest count
    assert _cons([A5, C5, A5], [(1, 2, E("GT"), 0, 3), (1, 0, 0, 1, 9)]) == ("ACGTA", [0, 5], [5], [[1, 2]])
    assert _cons([A5, C5, A5], [(1, 0, 0, 1, 9)]) == ("ACA", [0, 3], [3], [[0, 0]])
    # ties on the count: the shorter; then the smaller code; a higher count beats both
    assert _cons([A5], [(0, 1, E("T"), 0, 2), (0, 2, E("AA"), 0, 2)])[0] == "AT"
    assert _cons([A5], [(0, 2, E("CA"), 0, 2), (0, 2, E("AC"), 0, 2)])[0] == "AAC"
    assert _cons([A5], [(0, 1, E("T"), 0, 2), (0, 2, E("AA"), 0, 2), (0, 3, E("GGG"), 0, 3)])[0] == "AGGG"
    # a LOW anchor calls nothing; a DEL-called anchor's insertion stands in the letter's place
    assert _cons([A5, LOW, A5], [(1, 1, E("G"), 0, 4)]) == ("ANA", [0, 3], [3], [[0, 0]])
    assert _cons([A5, C5, A5], [(1, 1, E("G"), 0, 4)], min_depth=6) == ("NNN", [0, 3], [3], [[0, 0]])
    assert _cons([A5, D5, C5], [(1, 2, E("GG"), 0, 4)]) == ("AGGC", [0, 4], [4], [[1, 2]])
    assert _cons([D5, D5], [(0, 1, E("T"), 0, 1), (1, 1, E("G"), 0, 1)]) == ("TG", [0, 2], [2], [[2, 2]])
    # qualifies at equality and one below: min_count, then call_ppm against the anchor's depth (5)
    rows = [(0, 1, E("T"), 0, 2)]
    assert _cons([A5], rows, min_count=2)[0] == "AT" and _cons([A5], rows, min_count=3)[0] == "A"
    assert _cons([A5], rows, call_ppm=400000)[0] == "AT"               # 2 of 5 = 400 000 ppm exactly
    assert _cons([A5], rows, call_ppm=400001)[0] == "A"
    assert _cons([A5], rows, min_count=0, min_depth=0)[0] == "AT"      # 0 acts as 1
    # only the top allele is tested: a second one that would qualify is not called in its place
    assert _cons([A5], [(0, 1, E("T"), 0, 3), (0, 1, E("G"), 0, 2)], min_count=2)[0] == "AT"
    # segments: consecutive anchors, first and last position, a duplicated segment, an empty one
    got = _cons([A5, C5, A5, C5], [(0, 1, E("G"), 0, 1), (1, 1, E("T"), 0, 1), (2, 2, E("CC"), 0, 1),
                                   (3, 1, E("A"), 0, 1)], seg_off=[0, 2, 2, 4])
    assert got == ("AGCTACCCA", [0, 4, 4, 9], [4, 0, 5], [[2, 2], [0, 0], [2, 3]])


# ------------------------------------------------------------------ writers

def test_write_insertions_bytes():
    from metacov_amd import bases as mb
    fh = io.StringIO()
    ins = mb.Insertions([0, 3], [4, 4, 9], [2, 0, 32], [E("GT"), 0, E("ACGT" * 8)], [0, 1, 0], [3, 1, 2])
    seqs = [ins.sequence(k) for k in range(3)]
    assert seqs == ["GT", "*", "ACGT" * 8]
    assert mb.write_insertions(fh, "c 1", [104, 104, 109], [8, 8, 5], ins.count, ins.length, seqs) == 3
    assert fh.getvalue() == ("c 1\t105\t8\t3\t2\tGT\nc 1\t105\t8\t1\t0\t*\nc 1\t110\t5\t2\t32\t%s\n" % ("ACGT" * 8))
    assert mb.INSERTIONS_HEADER == im.HEADER == "contig\tpos\tdepth\tcount\tlen\tseq\n"
    # the model's writer gives the same bytes
    planes = np.zeros((6, 10), np.uint32)
    planes[bm.A, 4], planes[bm.DEL, 9] = 8, 5
    t = im.make_table([(4, 2, E("GT"), 0, 3), (4, 0, 0, 1, 1), (9, 32, E("ACGT" * 8), 0, 2)])
    assert im.tsv(["c 1"], [0], [100], [0, 10], planes, t, header=False) == fh.getvalue()
    assert mb.write_insertions(io.StringIO(), "x", [], [], [], [], []) == 0


def test_write_summary_with_insertions_bytes():
    from metacov_amd import bases as mb
    rows = np.array([[10, 5, 1, 1, 2, 1, 3, 12], [0] * 8], np.int64)
    extra = np.array([[2, 3], [0, 0]], np.int64)
    fh = io.StringIO()
    assert mb.write_consensus_summary(fh, ["c1", "c2"], [0, 7], [10, 7], rows, inserted=extra) == 2
    assert fh.getvalue() == ("contig\tstart\tend\tpositions\tcalled\tambiguous\tnocall\tlow\tdeleted\tdiffers\t"
                             "length\tinsertions\tinserted\nc1\t0\t10\t10\t5\t1\t1\t2\t1\t3\t12\t2\t3\n"
                             "c2\t7\t7\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\n")
    assert fh.getvalue() == im.summary_table([("c1", 0, 10, rows[0], extra[0]), ("c2", 7, 7, rows[1], extra[1])])
    fh = io.StringIO()                                                 # without them: the bytes of before
    mb.write_consensus_summary(fh, ["c1"], [0], [10], rows[:1])
    assert fh.getvalue() == cm.summary_table([("c1", 0, 10, rows[0])])


# ---------------------------------------------------------------------- CLI

def test_cli_option_errors(golden_dir, tmp_path):
    from metacov_amd.cli import main
    bam = os.path.join(golden_dir, "synth_exp.bam")
    r = CliRunner().invoke(main, ["consensus", "-b", bam, "--insertions", "--aligned"])
    assert r.exit_code == 2 and "--insertions" in r.output and "aligned" in r.output
    r = CliRunner().invoke(main, ["bases", "-b", bam, "--insertions"])                 # needs a file name
    assert r.exit_code == 2 and "--insertions" in r.output
    r = CliRunner().invoke(main, ["bases", "-b", bam, "--insertions", str(tmp_path / "i.tsv"), "--min-frac", "2"])
    assert r.exit_code == 2 and "min-frac" in r.output
    for cmd in ("bases", "consensus"):
        r = CliRunner().invoke(main, [cmd, "--help"])
        assert r.exit_code == 0 and "--insertions" in r.output
    from metacov_amd import bases as mb
    with pytest.raises(ValueError):
        mb.consensus(bam, "x", aligned=True, insertions=True)


def test_abi_table_has_insertions():
    for name in ("mc_bases_track_insertions", "mc_bases_insertions", "mc_bases_insertions_first",
                 "mc_bases_insertions_get", "mc_bases_insertions_timing", "mc_bases_ins_set",
                 "mc_bases_consensus_ins"):
        assert name in _lib.SIGNATURES
