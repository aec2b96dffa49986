"""The comparison contract without a GPU: the numpy model (tests/compare_model.py)
against a per-position pure-Python loop and against exact rational arithmetic,
the 2^26 bound, symmetry, the reduction to the diversity model, the writer's
bytes, the command's option errors and the ctypes table."""
import io
import os
from fractions import Fraction

import numpy as np
import pytest
from click.testing import CliRunner

from metacov_amd import _lib
from tests import compare_model as cm
from tests import diversity_model as dm


def random_pair(rng, n, hi=6, mc=2, ppm=250000):
    """Two plane sets with what the rule turns on: ties for the major allele,
    minor counts on the min_count and min_ppm edges, positions covered in one
    sample only, empty and monomorphic positions, the same and other majors."""
    out = []
    for _ in range(2):
        p = rng.integers(0, hi, size=(6, n)).astype(np.uint32)
        p[:, rng.random(n) < 0.15] = 0
        k = rng.random(n) < 0.3                                   # monomorphic
        p[1:4, k] = 0
        k = np.flatnonzero(rng.random(n) < 0.15)                  # a tie of two channels at the top
        c = rng.integers(0, 3, size=len(k))
        p[c, k] = p[c + 1, k] = hi
        k = np.flatnonzero(rng.random(n) < 0.15)                  # minor = mc, or one below, at ppm of n exactly
        if ppm:
            minor = np.where(rng.random(len(k)) < 0.5, mc, max(mc - 1, 0))
            total = minor * 1000000 // ppm + rng.integers(0, 2, size=len(k))     # on the edge, or one past it
            p[:4, k] = 0
            p[0, k] = np.maximum(total - minor, 0)
            p[int(rng.integers(1, 4)), k] = minor
        out.append(p)
    a, b = out
    a[:4, rng.random(n) < 0.1] = 0                                # covered in b only (where b is)
    b[:4, rng.random(n) < 0.1] = 0
    k = rng.random(n) < 0.1                                       # the same counts in both
    b[:, k] = a[:, k]
    return a, b


@pytest.mark.parametrize("seed", range(6))
def test_model_against_loop(seed):
    rng = np.random.default_rng(40 + seed)
    seg_off = np.cumsum([0, 1, 0, 37, 64, 5, 5])
    n = int(seg_off[-1])
    kw = dict(min_depth=int(rng.integers(0, 6)), min_count=int(rng.integers(0, 4)),
              min_ppm=int(rng.choice([0, 50000, 333333, 1000000])))
    a, b = random_pair(rng, n, hi=int(rng.choice([3, 6, 50, 100000])), mc=max(kw["min_count"], 1),
                       ppm=kw["min_ppm"])
    per = cm.per_position(a, b, **kw)
    for window in (0, 16, 17, 40):
        f1, r1 = cm.compare_model(a, b, seg_off, window, **kw)
        f2, r2 = cm.loop_model(a, b, seg_off, window, **kw)
        assert np.array_equal(f1, f2) and np.array_equal(r1, r2), (window, kw)
        assert r1[:, cm.POSITIONS].sum() == n
    assert (per[cm.POP_DIFF] <= per[cm.CON_DIFF]).all()                  # no shared allele: the majors differ
    assert (per[cm.COMPARED] <= per[cm.COVERED_A]).all() and (per[cm.COMPARED] <= per[cm.COVERED_B]).all()
    whole = cm.compare_model(a, b, seg_off, 0, **kw)[1]
    by16 = cm.compare_model(a, b, seg_off, 16, **kw)
    for s in range(len(seg_off) - 1):                                    # windows add up to their segment
        part = by16[1][by16[0][s]:by16[0][s + 1]].sum(axis=0)
        if seg_off[s + 1] > seg_off[s]:
            assert np.array_equal(part, whole[dm.windows(seg_off, 0)[0][s]])


def test_generator_reaches_the_edges():
    """What random_pair promises is there: the cases the rule turns on."""
    rng = np.random.default_rng(3)
    a, b = random_pair(rng, 4000, hi=6, mc=2, ppm=250000)
    kw = dict(min_depth=3, min_count=2, min_ppm=250000)
    per = cm.per_position(a, b, **kw)
    top = np.sort(a[:4].astype(np.int64), axis=0)
    assert ((top[3] == top[2]) & (top[3] > 0)).sum() > 100                       # ties for the major allele
    n = a[:4].astype(np.int64).sum(axis=0)
    assert ((top[2] == 2) & (top[2] * 1000000 == 250000 * n)).sum() > 20         # both edges at once
    assert ((top[2] == 1) & (n >= 3)).sum() > 20                                 # below min_count
    assert ((per[cm.COVERED_A] == 1) & (per[cm.COVERED_B] == 0)).sum() > 100
    assert ((per[cm.COVERED_A] == 0) & (per[cm.COVERED_B] == 1)).sum() > 100
    for col in (cm.COMPARED, cm.CON_DIFF, cm.POP_DIFF, cm.SNV, cm.DIST_FIX):
        assert per[col].any()
    assert ((per[cm.CON_DIFF] == 1) & (per[cm.POP_DIFF] == 0)).any()


def test_q_against_exact_rational():
    rng = np.random.default_rng(5)
    pairs = [(rng.integers(0, 1 << int(rng.integers(1, 25)), size=4), rng.integers(0, 1 << int(rng.integers(1, 25)),
                                                                                   size=4)) for _ in range(3000)]
    fixed = [((5, 0, 0, 0), (0, 7, 0, 0)),                       # disjoint alleles: 2^32 exactly
             ((3, 4, 0, 0), (0, 0, 9, 1)),
             (((1 << 26) - 1, 0, 0, 0), (0, 0, 0, (1 << 26) - 1)),
             ((2, 1, 0, 0), (4, 2, 0, 0)),                       # proportional: 0
             ((1, 1, 1, 1), (7, 7, 7, 7)),
             ((1 << 25, (1 << 25) - 1, 0, 0), ((1 << 25) - 1, 1 << 25, 0, 0)),
             ((1, 1, 0, 0), (1, 0, 1, 0))]                       # half the mass moves
    pairs += fixed
    a, b = np.zeros((6, len(pairs)), np.uint32), np.zeros((6, len(pairs)), np.uint32)
    a[:4] = np.array([p[0] for p in pairs], np.int64).T
    b[:4] = np.array([p[1] for p in pairs], np.int64).T
    per = cm.per_position(a, b)
    seen = 0
    for i, (x, y) in enumerate(pairs):
        x, y = [int(v) for v in x], [int(v) for v in y]
        nx, ny = sum(x), sum(y)
        if nx < 2 or ny < 2:
            assert per[cm.DIST_FIX, i] == 0 and per[cm.COMPARED, i] == 0
            continue
        seen += 1
        exact = Fraction(sum(abs(x[c] * ny - y[c] * nx) for c in range(4)) << 32, 2 * nx * ny)
        assert abs(int(per[cm.DIST_FIX, i]) - round(exact)) <= 1, (x, y)
        assert 0 <= per[cm.DIST_FIX, i] <= cm.ONE
        assert per[cm.DIST_FIX, i] == cm.position_loop(x, y)[cm.DIST_FIX]
    assert seen > 2900
    k = len(pairs) - len(fixed)
    assert per[cm.DIST_FIX, k:k + 3].tolist() == [cm.ONE] * 3
    assert per[cm.POP_DIFF, k:k + 3].tolist() == [1, 1, 1]
    assert per[cm.DIST_FIX, k + 3:k + 5].tolist() == [0, 0]
    assert per[cm.DIST_FIX, k + 6] == cm.ONE // 2


def test_bound_on_n():
    big = (1 << 26) - 1
    a, b = np.zeros((6, 4), np.uint32), np.zeros((6, 4), np.uint32)
    a[0, 1], a[1, 1] = 1 << 25, (1 << 25) - 1                     # n_a = n_b = 2^26 - 1: accepted
    b[3, 1] = big
    first, rows = cm.compare_model(a, b, [0, 4])
    assert rows[0].tolist() == [4, 1, 1, 1, 1, 1, 1, cm.ONE]
    assert rows.tolist() == cm.loop_model(a, b, [0, 4])[1].tolist()
    for which in (0, 1):                                          # 2^26 in either sample: the lowest index
        x, y = a.copy(), b.copy()
        deep, other = (x, y) if which == 0 else (y, x)
        deep[2, 3], other[2, 3] = 1 << 26, 5
        deep[0, 2], other[1, 2] = 1 << 27, 2
        with pytest.raises(cm.RangeError) as e:
            cm.compare_model(x, y, [0, 4])
        assert e.value.index == 2
        with pytest.raises(cm.RangeError):
            cm.position_loop(x[:4, 2], y[:4, 2])
        other[:4, 2:] = 0                                         # the other sample uncovered there: no error
        other[0, 2] = 1
        rows = cm.compare_model(x, y, [0, 4])[1]
        assert rows[0, cm.COMPARED] == 1 and rows[0, 1 + which] == 3 and rows[0, 2 - which] == 1
        assert rows.tolist() == cm.loop_model(x, y, [0, 4])[1].tolist()


def test_symmetry():
    rng = np.random.default_rng(11)
    a, b = random_pair(rng, 500)
    for kw in (dict(), dict(min_depth=4, min_count=2, min_ppm=250000)):
        for window in (0, 16, 33):
            f1, ab = cm.compare_model(a, b, [0, 200, 500], window, **kw)
            f2, ba = cm.compare_model(b, a, [0, 200, 500], window, **kw)
            assert np.array_equal(f1, f2)
            assert np.array_equal(ab[:, [0, 2, 1, 3, 4, 5, 6, 7]], ba)
            assert ab[:, cm.DIST_FIX].any() and (ab[:, 1] != ab[:, 2]).any()


def one_hot_reference(ref, md):
    """The planes of a sample that shows the reference base md times where its code is known."""
    ref = np.asarray(ref)
    b = np.zeros((6, len(ref)), np.uint32)
    known = np.flatnonzero(ref < 4)
    b[ref[known], known] = md
    return b


def test_reduction_to_diversity():
    rng = np.random.default_rng(12)
    n = 700
    a, _ = random_pair(rng, n)
    ref = rng.integers(0, 6, size=n).astype(np.uint8)
    for kw in (dict(), dict(min_depth=3, min_count=2, min_ppm=250000), dict(min_depth=5, min_count=1, min_ppm=400000)):
        b = one_hot_reference(ref, max(kw.get("min_depth", 2), 2))
        for window in (0, 16, 100):
            f1, rows = cm.compare_model(a, b, [0, 1, 300, n], window, **kw)
            f2, div = dm.diversity_model(a, [0, 1, 300, n], window, ref=ref, **kw)
            assert np.array_equal(f1, f2)
            assert np.array_equal(rows[:, [cm.COMPARED, cm.CON_DIFF, cm.POP_DIFF]],
                                  div[:, [dm.COMPARED, dm.CON_DIFF, dm.POP_DIFF]])
            assert div[:, dm.POP_DIFF].any() and (div[:, dm.CON_DIFF] > div[:, dm.POP_DIFF]).any()


def test_write_compare_bytes():
    from metacov_amd import bases as mb
    rows = np.array([[16, 12, 10, 8, 2, 1, 3, 3 << 31],            # the identities 0.75 and 0.875, af_dist 0.1875
                     [4, 3, 0, 0, 0, 0, 0, 0],                     # nothing compared: three NA
                     [7, 7, 7, 7, 0, 0, 0, 0]], np.int64)          # compared and identical
    d = mb.Comparison([0, 2, 2, 3], rows, window=16)
    assert len(d) == 3 and d.segment().tolist() == [0, 0, 2]
    assert d.start().tolist() == [0, 16, 0] and d.end().tolist() == [16, 20, 7]
    assert d.covered_a.tolist() == [12, 3, 7] and d.covered_b.tolist() == [10, 0, 7]
    assert d.snv.tolist() == [3, 0, 0] and d.dist_fix[0] == 3 << 31
    assert d.breadth_a().tolist() == [0.75, 0.75, 1.0] and d.breadth_b().tolist() == [0.625, 0.0, 1.0]
    assert d.overlap().tolist() == [0.5, 0.0, 1.0]
    assert d.con_ani()[0] == 0.75 and d.pop_ani()[0] == 0.875 and np.isnan(d.con_ani()[1]) and d.pop_ani()[2] == 1.0
    assert d.distance()[0] == 0.1875 and np.isnan(d.distance()[1]) and d.distance()[2] == 0
    assert d.distance().dtype == np.float64
    fh = io.StringIO()
    assert mb.write_compare(fh, ["c 1", "e", "c2"], [100, 0, 5], d) == 3
    want = ("#contig\tstart\tend\tpositions\tcovered_a\tcovered_b\tcompared\tcon_diff\tpop_diff\tsnv\tcon_ani\tpop_ani\t"
            "af_dist\n"
            "c 1\t100\t116\t16\t12\t10\t8\t2\t1\t3\t0.750000\t0.875000\t0.187500\n"
            "c 1\t116\t120\t4\t3\t0\t0\t0\t0\t0\tNA\tNA\tNA\n"
            "c2\t5\t12\t7\t7\t7\t7\t0\t0\t0\t1.000000\t1.000000\t0.000000\n")
    assert fh.getvalue() == want
    assert mb.COMPARE_HEADER == cm.HEADER == want.split("\n")[0] + "\n"
    assert cm.tsv(["c 1", "e", "c2"], [100, 0, 5], [0, 20, 20, 27], 16, d.win_first, rows) == want
    fh = io.StringIO()
    assert mb.write_compare(fh, [], [], mb.Comparison([0], np.zeros((0, 8), np.int64)), header=False) == 0
    assert fh.getvalue() == ""
    whole = mb.Comparison([0, 1], rows[:1])                        # window 0: the row starts its segment
    assert whole.start().tolist() == [0]
    assert mb.CMP_COLS == cm.COLS == len(mb.CMP_COLUMNS)


def test_cli_option_errors(golden_dir, tmp_path):
    from metacov_amd.cli import COMPARE_GROUP_POSITIONS, main
    bam = os.path.join(golden_dir, "synth_exp.bam")
    other = os.path.join(golden_dir, "bbmap.sorted.bam")
    r = CliRunner().invoke(main, ["compare", "-b", bam, "-c", bam, "--by", "5"])
    assert r.exit_code == 2 and "--by" in r.output and "16" in r.output
    r = CliRunner().invoke(main, ["compare", "-b", bam, "-c", bam, "--min-frac", "2"])
    assert r.exit_code == 2 and "min-frac" in r.output
    rc = tmp_path / "r.csv"
    rc.write_text("sequence_id,start,stop\n")
    r = CliRunner().invoke(main, ["compare", "-b", bam, "-c", bam, "-rc", str(rc), "-rb", str(rc)])
    assert r.exit_code == 2 and "Only one of" in r.output
    r = CliRunner().invoke(main, ["compare", "-b", bam, "-c", bam], env={"WORLD_SIZE": "2"})
    assert r.exit_code == 2 and "one process" in r.output
    r = CliRunner().invoke(main, ["compare", "-b", bam])
    assert r.exit_code == 2 and "-c" in r.output
    r = CliRunner().invoke(main, ["compare", "--help"])
    assert r.exit_code == 0 and "--by" in r.output and "--min-frac" in r.output and "-c" in r.output
    assert COMPARE_GROUP_POSITIONS == 1 << 29
    from metacov_amd import bases as mb
    with pytest.raises(ValueError):
        mb.compare(bam, bam, "x", window=5)
    with pytest.raises(ValueError):
        mb.compare(bam, bam, "x", decode="nowhere")
    # two files that do not share one reference: refused with the first difference, before the GPU is touched
    r = CliRunner().invoke(main, ["compare", "-b", bam, "-c", other])
    assert r.exit_code == 1 and "do not share one reference" in r.output and "synth_exp.bam" in r.output
    with pytest.raises(ValueError, match="reference"):
        mb.compare(bam, other, "x")


def test_header_mismatch_names_the_first_difference(tmp_path):
    from metacov_amd import bases as mb
    from metacov_amd import synth
    from metacov_amd.cli import main
    paths = []
    for k, (names, lengths) in enumerate(((["c1", "c2", "c3"], [500, 600, 700]), (["c1", "c2", "c3"], [500, 601, 700]),
                                          (["c1", "cX", "c3"], [500, 600, 700]), (["c1", "c2"], [500, 600]))):
        paths.append(str(tmp_path / ("h%d.bam" % k)))
        synth.write_bam(paths[-1], names, lengths, [synth.SynthRecord("r", 0, 10, 0, [(0, 4)], 4, seq="ACGT")])
    assert mb.same_references("x", ["c1"], [5], "y", ["c1"], [5]) is None
    r = CliRunner().invoke(main, ["compare", "-b", paths[0], "-c", paths[1]])
    assert r.exit_code == 1 and "reference 1" in r.output and "600 bp" in r.output and "601 bp" in r.output
    r = CliRunner().invoke(main, ["compare", "-b", paths[0], "-c", paths[2]])
    assert r.exit_code == 1 and "reference 1" in r.output and "'cX'" in r.output
    r = CliRunner().invoke(main, ["compare", "-b", paths[0], "-c", paths[3]])
    assert r.exit_code == 1 and "3 references" in r.output and "2" in r.output


def test_abi_table_has_compare():
    for name in ("mc_bases_compare", "mc_bases_compare_first", "mc_bases_compare_get", "mc_bases_compare_device",
                 "mc_bases_compare_timing"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mc_bases_compare"]) == 7
    assert _lib.SIGNATURES["mc_bases_compare_get"] == _lib.SIGNATURES["mc_bases_diversity_get"]
