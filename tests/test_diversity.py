"""The diversity contract without a GPU: the numpy model (tests/diversity_model.py)
against a per-position pure-Python loop and against exact rational arithmetic,
the 2^26 bound, pi <= 1, the writer's bytes, the command's option errors and
the ctypes table."""
import io
import os
from fractions import Fraction

import numpy as np
import pytest
from click.testing import CliRunner

from metacov_amd import _lib
from tests import diversity_model as dm


def random_planes(rng, n, hi=6):
    planes = rng.integers(0, hi, size=(6, n)).astype(np.uint32)
    planes[:, rng.random(n) < 0.15] = 0
    k = rng.random(n) < 0.3                     # monomorphic positions, as most of real data
    planes[1:4, k] = 0
    return planes


@pytest.mark.parametrize("seed", range(6))
def test_model_against_loop(seed):
    rng = np.random.default_rng(seed)
    seg_off = np.cumsum([0, 1, 0, 37, 64, 5, 5])
    n = int(seg_off[-1])
    planes = random_planes(rng, n, hi=int(rng.choice([3, 6, 50, 100000])))
    ref = rng.integers(0, 6, size=n).astype(np.uint8) if seed % 2 else None
    kw = dict(min_depth=int(rng.integers(0, 6)), min_count=int(rng.integers(0, 4)),
              min_ppm=int(rng.choice([0, 50000, 333333, 1000000])))
    for window in (0, 16, 17, 40):
        f1, r1 = dm.diversity_model(planes, seg_off, window, ref=ref, **kw)
        f2, r2 = dm.loop_model(planes, seg_off, window, ref=ref, **kw)
        assert np.array_equal(f1, f2) and np.array_equal(r1, r2), (window, kw)
        assert r1[:, dm.POSITIONS].sum() == n
        if ref is None:
            assert not r1[:, dm.COMPARED:].any()
    whole = dm.diversity_model(planes, seg_off, 0, ref=ref, **kw)[1]
    by16 = dm.diversity_model(planes, seg_off, 16, ref=ref, **kw)
    for s in range(len(seg_off) - 1):           # windows add up to their segment
        part = by16[1][by16[0][s]:by16[0][s + 1]].sum(axis=0)
        if seg_off[s + 1] > seg_off[s]:
            assert np.array_equal(part, whole[dm.windows(seg_off, 0)[0][s]])


def test_windows():
    first, seg, lo, hi = dm.windows([0, 0, 5, 5, 45], 16)
    assert first.tolist() == [0, 0, 1, 1, 4] and seg.tolist() == [1, 3, 3, 3]
    assert lo.tolist() == [0, 5, 21, 37] and hi.tolist() == [5, 21, 37, 45]
    assert dm.windows([0, 0, 5], 0)[0].tolist() == [0, 0, 1]
    with pytest.raises(ValueError):
        dm.windows([0, 5], 15)


def test_q_within_one_of_exact_rational():
    rng = np.random.default_rng(5)
    cols = [rng.integers(0, 1 << int(rng.integers(1, 25)), size=4) for _ in range(3000)]
    cols += [(1 << 25, (1 << 25) - 1, 0, 0), (1, 1, 0, 0), (1, 1, 1, 1), (3, 0, 0, 1), ((1 << 26) - 2, 1, 0, 0)]
    planes = np.zeros((6, len(cols)), np.uint32)
    planes[:4] = np.array(cols, np.int64).T
    per = dm.per_position(planes)
    for i, a in enumerate(cols):
        a = [int(x) for x in a]
        n = sum(a)
        if n < 2:
            assert per[dm.PI_FIX, i] == 0
            continue
        exact = Fraction(n * n - sum(x * x for x in a) << 32, n * (n - 1))
        assert abs(int(per[dm.PI_FIX, i]) - round(exact)) <= 1, a
        assert 0 <= per[dm.PI_FIX, i] <= dm.ONE
        assert per[dm.PI_FIX, i] == dm.position_loop(a, None)[dm.PI_FIX]
    assert per[dm.PI_FIX, len(cols) - 4] == dm.ONE               # (1, 1, 0, 0): every pair differs


def test_bound_on_n():
    planes = np.zeros((6, 3), np.uint32)
    planes[0, 1], planes[1, 1] = 1 << 25, (1 << 25) - 1           # n = 2^26 - 1
    first, rows = dm.diversity_model(planes, [0, 3])
    assert rows[0, dm.BASES] == (1 << 26) - 1 and rows[0, dm.COVERED] == 1
    assert rows.tolist() == dm.loop_model(planes, [0, 3])[1].tolist()
    planes[1, 1] += 1                                             # n = 2^26
    planes[2, 2] = 1 << 27
    with pytest.raises(dm.RangeError) as e:
        dm.diversity_model(planes, [0, 3])
    assert e.value.index == 1
    with pytest.raises(dm.RangeError):
        dm.position_loop(planes[:4, 1], None)
    rows = dm.diversity_model(planes, [0, 3], min_depth=(1 << 27) + 1)[1]     # below min_depth: not an error
    assert rows[0].tolist() == [3, 0, (1 << 26) + (1 << 27), 0, 0, 0, 0, 0]


def test_pi_at_most_one():
    rng = np.random.default_rng(9)
    planes = np.zeros((6, 20000), np.uint32)
    planes[:4] = rng.integers(0, 40, size=(4, 20000))
    planes[:4, ::3] = rng.integers(0, 3, size=planes[:4, ::3].shape)
    per = dm.per_position(planes)
    assert per[dm.PI_FIX].max() == dm.ONE and per[dm.PI_FIX].min() == 0
    first, rows = dm.diversity_model(planes, [0, 20000], 16)
    assert (rows[:, dm.PI_FIX] <= rows[:, dm.COVERED] * dm.ONE).all()


def test_write_diversity_bytes():
    from metacov_amd import bases as mb
    rows = np.array([[16, 10, 55, 2, 3 << 31, 8, 2, 1],           # pi = 0.15, the identities 0.75 and 0.875
                     [4, 0, 3, 0, 0, 0, 0, 0],                    # nothing covered: three NA
                     [7, 7, 70, 0, 0, 0, 0, 0]], np.int64)        # covered, no reference: pi 0, the identities NA
    d = mb.Diversity([0, 2, 2, 3], rows, window=16)
    assert len(d) == 3 and d.segment().tolist() == [0, 0, 2]
    assert d.start().tolist() == [0, 16, 0] and d.end().tolist() == [16, 20, 7]
    assert d.covered.tolist() == [10, 0, 7] and d.pop_diff.tolist() == [1, 0, 0]
    assert d.pi()[0] == 0.15 and np.isnan(d.pi()[1]) and d.pi()[2] == 0
    assert d.breadth().tolist() == [0.625, 0.0, 1.0] and d.mean_depth()[2] == 10
    assert d.snv_density()[0] == 0.2 and np.isnan(d.snv_density()[1])
    assert d.con_ani()[0] == 0.75 and d.pop_ani()[0] == 0.875 and np.isnan(d.con_ani()[2])
    assert d.pi().dtype == np.float64
    fh = io.StringIO()
    assert mb.write_diversity(fh, ["c 1", "e", "c2"], [100, 0, 5], d) == 3
    want = ("#contig\tstart\tend\tpositions\tcovered\tbases\tsnv\tpi\tcompared\tcon_diff\tpop_diff\tcon_ani\tpop_ani\n"
            "c 1\t100\t116\t16\t10\t55\t2\t0.150000\t8\t2\t1\t0.750000\t0.875000\n"
            "c 1\t116\t120\t4\t0\t3\t0\tNA\t0\t0\t0\tNA\tNA\n"
            "c2\t5\t12\t7\t7\t70\t0\t0.000000\t0\t0\t0\tNA\tNA\n")
    assert fh.getvalue() == want
    assert mb.DIVERSITY_HEADER == dm.HEADER == want.split("\n")[0] + "\n"
    assert dm.tsv(["c 1", "e", "c2"], [100, 0, 5], [0, 20, 20, 27], 16, d.win_first, rows) == want
    fh = io.StringIO()
    assert mb.write_diversity(fh, [], [], mb.Diversity([0], np.zeros((0, 8), np.int64)), header=False) == 0
    assert fh.getvalue() == ""
    whole = mb.Diversity([0, 1], rows[:1])                         # window 0: the row starts its segment
    assert whole.start().tolist() == [0]


def test_cli_option_errors(golden_dir, tmp_path):
    from metacov_amd.cli import main
    bam = os.path.join(golden_dir, "synth_exp.bam")
    r = CliRunner().invoke(main, ["diversity", "-b", bam, "--by", "5"])
    assert r.exit_code == 2 and "--by" in r.output and "16" in r.output
    r = CliRunner().invoke(main, ["diversity", "-b", bam, "--min-frac", "2"])
    assert r.exit_code == 2 and "min-frac" in r.output
    rc = tmp_path / "r.csv"
    rc.write_text("sequence_id,start,stop\n")
    r = CliRunner().invoke(main, ["diversity", "-b", bam, "-rc", str(rc), "-rb", str(rc)])
    assert r.exit_code == 2 and "Only one of" in r.output
    r = CliRunner().invoke(main, ["diversity", "-b", bam], env={"WORLD_SIZE": "2"})
    assert r.exit_code == 2 and "one process" in r.output
    r = CliRunner().invoke(main, ["diversity", "--help"])
    assert r.exit_code == 0 and "--by" in r.output and "--min-frac" in r.output
    from metacov_amd import bases as mb
    with pytest.raises(ValueError):
        mb.diversity(bam, "x", window=5)
    with pytest.raises(ValueError):
        mb.diversity(bam, "x", decode="nowhere")


def test_abi_table_has_diversity():
    for name in ("mc_bases_diversity", "mc_bases_diversity_first", "mc_bases_diversity_get",
                 "mc_bases_diversity_device", "mc_bases_diversity_timing"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mc_bases_diversity"]) == 7
