"""CPU checks of the cases of tests/test_gpu_device_rows.py
(tests/device_rows_cases.py): every case whose meaning depends on an engine
path must still reach it.  A change of the engine's constants then fails
here, by name, and not on the GPU as a case that silently took another path."""
import numpy as np
import pytest

from tests import device_rows_cases as dc
from tests import fused_model as fm


def ceil_div(a, b):
    return -(-a // b)


def test_constants_match_source():
    src = fm.source_constants()
    assert fm.K_LDS_BINS == src["K_LDS_BINS"] and fm.K_FB_SLOTS == src["K_FB_SLOTS"]
    assert dc.source_max_hist() == 1 << 28
    assert dc.HIST_SWITCH_DEPTHS == (src["K_LDS_BINS"] - 1, src["K_LDS_BINS"], src["K_LDS_BINS"] + 1)


def test_table_geometry():
    """The two leads put the first row on a 16-byte boundary and off it (the
    allocation itself is at least 16-byte aligned)."""
    assert sorted((lead * dc.ROW_WORDS * 8) % 16 for lead in dc.LEADS) == [0, 8]
    assert dc.TAIL > 0 and min(dc.LEADS) > 0


@pytest.mark.parametrize("empty", [False, True])
def test_short_case_fits_the_direct_path(empty):
    """Sorted short reads inside their contigs; no region leaves its window
    (the repeated call's clean-buffer path needs a call without recomputes)."""
    c = dc.short_case(empty=empty)
    d, ext, coff = c.depth()
    assert np.array_equal(ext, c.lengths) and int(c.span.max()) <= fm.K_SHORT_MAX
    assert (np.diff(coff[c.tid] + c.pos) >= 0).all()
    assert int(d.max()) < fm.K_HIST_BINS
    for variant in ("direct", "full"):
        base, flags = dc.model_flags(c, variant)
        assert (base == 0).all() and not flags.any(), variant
    if empty:
        assert (c.tid < len(c.lengths) - 1).all() and c.lengths[-1] == dc.EMPTY_CONTIG


@pytest.mark.parametrize("seed", [77, 78])
def test_long_case_is_recomputed_on_the_device(seed):
    c = dc.long_case(seed)
    d, ext, coff = c.depth()
    assert int(c.span.max()) > fm.K_SHORT_MAX          # long reads: the device recompute is on from the first call
    assert int(d.max()) < fm.K_LDS_BINS - 1            # (below the piles of the switch test, too)
    _, flags = dc.model_flags(c, "full")
    assert 0 < flags.sum() <= fm.K_FB_SLOTS
    assert fm.recompute_path(int(flags.sum()), True, int(d.max())) == (0, int(flags.sum()))


@pytest.mark.parametrize("pile", [fm.K_LDS_BINS - 1, fm.K_LDS_BINS, 17_000])
def test_long_case_piles(pile):
    """The pile's contig holds nothing else, so the maximum depth is the
    pile; its region is flagged; the depth decides who recomputes."""
    c = dc.long_case(pile=pile)
    d, ext, coff = c.depth()
    assert int(d.max()) == pile == int(d[coff[dc.LONG_CONTIGS]:].max())
    _, flags = dc.model_flags(c, "full")
    assert flags[dc.LONG_CONTIGS] and flags.sum() <= fm.K_FB_SLOTS
    n = int(flags.sum())
    assert fm.recompute_path(n, True, pile) == ((0, n) if pile < fm.K_LDS_BINS else (n, 0))


@pytest.mark.parametrize("kind", ["direct", "recompute"])
def test_visibility_batches_differ_in_every_region(kind):
    """A stale row (the other batch's) cannot pass for the current one."""
    a, b = (dc.short_case(17), dc.short_case(18)) if kind == "direct" else (dc.long_case(77), dc.long_case(78))
    assert np.array_equal(a.lengths, b.lengths)
    assert all(np.array_equal(x, y) for x, y in zip(a.regions(), b.regions()))
    ra, rb = a.rows(), b.rows()
    assert len(ra) == len(rb) > 0
    for r in range(len(ra)):
        assert ra[r].tobytes() != rb[r].tobytes(), r
        assert int(ra[r]["sum"]) != int(rb[r]["sum"]), r


@pytest.mark.parametrize("variant", ["direct", "full"])
def test_slot_case_flags_one_more_than_the_slots(variant):
    c = dc.slot_case(variant)
    _, flags = dc.model_flags(c, variant)
    assert flags.sum() == fm.K_FB_SLOTS + 1
    for device_on in (False, True):
        assert fm.recompute_path(int(flags.sum()), device_on, int(c.depth()[0].max())) == (fm.K_FB_SLOTS + 1, 0)


def test_region_shapes():
    n = len(dc.short_case(empty=True).lengths)
    for name in dc.SHAPES:
        c = dc.shape_case(name)
        assert (c.rt >= 0).all() and (c.rt < n).all() and (c.rs >= 0).all() and (c.re >= c.rs).all(), name
        d, ext, coff = c.depth()
        gs, ge = coff[c.rt] + np.minimum(c.rs, ext[c.rt]), coff[c.rt] + np.minimum(c.re, ext[c.rt])
        o = np.argsort(gs, kind="stable")
        live = (ge > gs)[o]
        overlap = bool((gs[o][live][1:] < ge[o][live][:-1]).any())
        assert overlap == (name == "overlap"), name
    assert dc.shape_case("r1").R == 1 and dc.shape_case("r5").R == 5
    c = dc.shape_case("r1000")
    assert c.R == 1000 and (c.re - c.rs == 1).all() and (c.re <= c.lengths[c.rt]).all()
    c = dc.shape_case("zeros")
    ext = c.depth()[1]
    empty = c.rt == n - 1
    assert empty.any() and (~empty).any() and (c.rs[~empty] >= ext[c.rt[~empty]]).all()
    rows = c.rows()
    assert (rows["n"] > 0).all() and (rows["sum"] == 0).all() and (rows["max"] == 0).all()


@pytest.mark.parametrize("depth", dc.HIST_SWITCH_DEPTHS)
def test_histogram_switch_piles(depth):
    """Maximum depth exactly D: nbins = D + 1 sits on, and on both sides of,
    the switch `nbins <= kLdsBins`."""
    c = dc.pile_case(depth)
    d, ext, coff = c.depth()
    assert int(d.max()) == depth and ext[0] == c.lengths[0] == 1000
    assert (depth + 1 <= fm.K_LDS_BINS) == (depth == dc.HIST_SWITCH_DEPTHS[0])
    rows = c.rows()
    # the whole contig, a region that cuts the pile, one that misses it, one past the extent
    assert rows["max"].tolist() == [depth, depth, 0, 0] and rows["min"].tolist() == [0, 0, 0, 0]
    assert 0 < rows["sum"][1] < rows["sum"][0] and c.rs[3] >= ext[0] and rows["n"][3] > 0


def test_batch_plain_case_takes_three_batches():
    c = dc.batch_plain_case()
    d, ext, coff = c.depth()
    assert c.R == 9003 and int(d.max()) == dc.BATCH_DEPTH and ext[0] == 70_000
    rb = dc.region_batch(int(d.max()))
    assert rb == dc.source_max_hist() // (dc.BATCH_DEPTH + 1) == 4095
    assert ceil_div(c.R, rb) == 3
    rows = c.rows()
    # every batch has covered positions (one region_seg_kernel launch each) and one region over the pile
    for k in range(3):
        sel = slice(k * rb, min(c.R, (k + 1) * rb))
        assert (np.minimum(c.re[sel], ext[0]) > np.minimum(c.rs[sel], ext[0])).any()
        assert (rows["max"][sel] == dc.BATCH_DEPTH).any(), k
    # a row written at the wrong batch offset cannot pass: the rows of regions rb apart differ
    same = [r for r in range(c.R - rb) if rows[r].tobytes() == rows[r + rb].tobytes()]
    assert len(same) < c.R // 20, len(same)


def test_batch_fallback_case_is_recomputed_by_the_host_in_two_batches():
    c = dc.batch_fallback_case()
    d, ext, coff = c.depth()
    assert c.R == 5001 and int(d.max()) == dc.BATCH_DEPTH and ext[0] == c.lengths[0] == 20_000
    assert np.array_equal(fm.window_base_full(ext, c.tid, c.span), [689])
    assert np.array_equal(fm.window_base_direct(c.lengths, c.tid, c.span), [689])
    for variant in ("full", "direct"):
        base, flags = dc.model_flags(c, variant)
        assert base[0] == 689 and flags.all(), variant
    for device_on in (False, True):
        assert fm.recompute_path(5001, device_on, dc.BATCH_DEPTH) == (5001, 0)
    rb = dc.region_batch(int(d.max()))
    assert ceil_div(5001, rb) == 2 and 5001 - rb == 906
    # fusable: no two regions overlap
    o = np.argsort(c.rs)
    assert (c.rs[o][1:] >= c.re[o][:-1]).all()
