"""The device-output statistics calls (compute_depth_stats_device,
region_stats_device: what bench.py times and INTEGRATION.md §3 names as the
multi-GPU contract) and K3's region batching, on the GPU.

Every call writes into a sentinel-filled table with guard rows on both sides
of the destination, at a 16-byte aligned and an unaligned row address.  The
table is read back on a stream of the test's own, with no synchronise of the
engine's stream or the device between the call's return and the copy: the
rows must be in place and visible when the call returns.  Every field of
every row is compared with the oracle (exact integers, no tolerance), every
guard row must still hold the sentinel, and each case asserts the engine path
it took.  tests/test_device_rows_model.py checks on the CPU that the cases
reach those paths.

The clean-buffer path of a repeated call (no init launch) has no counter of
its own: its case asserts what selects it (no re-prepare, the same region
count, no recomputed region in the call before) and runs under
MC_CHECK_CLEAN=1 as well, where the engine verifies the skipped init.

The visibility test cannot be made to fail by a deterministic change of the
engine: it catches a missing or late row only when the race is lost.

Run on an MI355X:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest

from metacov_amd import synth
from metacov_amd._lib import MetacovError, MC_E_INVALID, MC_E_STATE
from metacov_amd.engine import CoverageEngine
from tests import device_rows_cases as dc
from tests import fused_model as fm

pytestmark = pytest.mark.gpu

ROW_BYTES = dc.ROW_WORDS * 8


@pytest.fixture(scope="module")
def torch_(lib_built):
    import torch
    return torch


@pytest.fixture
def side(torch_):
    """The test's own stream: sentinel fills and read-backs run here."""
    return torch_.cuda.Stream()


def load(eng, case, direct=True):
    if not direct:
        eng.set_direct_prepare(False)
    eng.set_contigs(case.lengths)
    eng.add_reads(case.tid, case.pos, case.span)


def run(torch, eng, side, case, lead, call="fused", regs=None, what=""):
    """One engine call into a guarded table, read back without a synchronise
    of the engine's stream, checked against the oracle."""
    rt, rs, re_ = regs if regs is not None else (case.rt, case.rs, case.re)
    want = case.rows() if regs is None else case.rows_of(rt, rs, re_)
    table, at = dc.guarded_table(torch, len(rt), lead, dc.TAIL, side)
    if call == "fused":
        eng.compute_depth_stats_device(rt, rs, re_, at)
    else:
        eng.compute_depth()
        eng.region_stats_device(rt, rs, re_, at)
    host = dc.read_back(torch, table, side)
    dc.check(host, lead, len(rt), want, (what, call, "lead %d" % lead))


def delta(t0, t1, *keys):
    return tuple(t1[k] - t0[k] for k in keys)


PREP = ("direct_batches", "full_prepares", "fused_calls")


# ------------------------------------------------ 1. every path, device destination

def _path_prepare(torch, eng, side, direct):
    case = dc.short_case()
    load(eng, case, direct)
    for lead in dc.LEADS:
        eng.invalidate()
        t0 = eng.timings()
        run(torch, eng, side, case, lead)
        assert delta(t0, eng.timings(), *PREP) == ((1, 0, 1) if direct else (0, 1, 1))
        assert (eng.fused_fallbacks(), eng.fused_recomputes()) == (0, 0)


def _path_reused(torch, eng, side):
    case = dc.short_case()
    load(eng, case)
    t0 = eng.timings()
    eng.prepare()
    for lead in dc.LEADS + dc.LEADS[:1]:      # the second and third call: clean buffers, both parities
        run(torch, eng, side, case, lead)
        assert (eng.fused_fallbacks(), eng.fused_recomputes()) == (0, 0)
    assert delta(t0, eng.timings(), *PREP) == (0, 1, 3)


def _path_recompute(torch, eng, side):
    case = dc.long_case()
    load(eng, case)
    for lead in dc.LEADS:
        run(torch, eng, side, case, lead)
        assert eng.fused_recomputes() > 0 and eng.fused_fallbacks() == 0
        assert eng.max_depth() < fm.K_LDS_BINS
    assert eng.timings()["direct_batches"] == 0


def _path_fallback_depth(torch, eng, side):
    case = dc.long_case(pile=17_000)
    load(eng, case)
    for lead in dc.LEADS:
        run(torch, eng, side, case, lead)
        assert eng.max_depth() > fm.K_LDS_BINS
        assert eng.fused_fallbacks() > 0 and eng.fused_recomputes() == 0


def _path_fallback_count(torch, eng, side, variant):
    case = dc.slot_case(variant)
    load(eng, case, variant == "direct")
    device_on = False
    for lead in dc.LEADS:
        run(torch, eng, side, case, lead)
        got = (eng.fused_fallbacks(), eng.fused_recomputes())
        assert got == fm.recompute_path(fm.K_FB_SLOTS + 1, device_on, eng.max_depth()) == (fm.K_FB_SLOTS + 1, 0)
        device_on = True      # (a call that flagged regions switches the device recompute on)
    t = eng.timings()
    assert (t["direct_batches"], t["full_prepares"]) == ((1, 0) if variant == "direct" else (0, 1))


def _path_shape(torch, eng, side, name):
    case = dc.shape_case(name)
    load(eng, case)
    for lead in dc.LEADS:
        eng.invalidate()
        t0 = eng.timings()
        run(torch, eng, side, case, lead, what=name)
        d = delta(t0, eng.timings(), "fused_calls", "stats_launches", "direct_batches")
        # overlapping regions are not fusable: K2, then one K3 pass
        assert d == ((0, 1, 1) if name == "overlap" else (1, 1, 1)), d
    if name == "zeros":
        rows = case.rows()
        assert (rows["n"] > 0).all() and all((rows[f] == 0).all() for f in rows.dtype.names if f not in ("n", "q23_cnt"))


def _path_r0(torch, eng, side):
    """No regions and a null pointer: K2 runs, nothing else is touched."""
    case = dc.short_case()
    load(eng, case)
    none = (np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64))
    table, _ = dc.guarded_table(torch, 0, 2, dc.TAIL, side)
    t0 = eng.timings()
    eng.compute_depth_stats_device(*none, 0)
    eng.region_stats_device(*none, 0)
    host = dc.read_back(torch, table, side)
    dc.check(host, 2, 0, case.rows()[:0], "R = 0")
    assert delta(t0, eng.timings(), "depth_launches", "stats_launches", "fused_calls") == (1, 0, 0)
    assert eng.max_depth() == int(case.depth()[0].max())


PATHS = {
    "direct": lambda *a: _path_prepare(*a, True),
    "full": lambda *a: _path_prepare(*a, False),
    "reused": _path_reused,
    "reused_checked": _path_reused,
    "recompute": _path_recompute,
    "fallback_depth": _path_fallback_depth,
    "fallback_count_direct": lambda *a: _path_fallback_count(*a, "direct"),
    "fallback_count_full": lambda *a: _path_fallback_count(*a, "full"),
    "r0": _path_r0,
}
for _name in dc.SHAPES:
    PATHS["shape_" + _name] = lambda *a, _name=_name: _path_shape(*a, _name)


@pytest.mark.parametrize("name", list(PATHS))
def test_every_path_device_destination(torch_, side, monkeypatch, name):
    """compute_depth_stats_device on every path of the fused call: exactly the
    R rows at the caller's pointer are written, and they are the oracle's."""
    if name == "reused_checked":
        monkeypatch.setenv("MC_CHECK_CLEAN", "1")     # read at mc_ctx_create
    eng = CoverageEngine(0)
    try:
        PATHS[name](torch_, eng, side)
    finally:
        eng.close()


# ------------------------------------------------ 2. rows visible on return

@pytest.mark.parametrize("kind", ["direct", "recompute"])
def test_rows_visible_on_return(torch_, side, kind):
    """32 steps that alternate two resident batches over the same contigs,
    each read back right after the call returns.  The destination holds the
    sentinel (first write) or the other batch's rows, which differ in every
    region, so a row that is not yet visible fails at its step.  The engine's
    stream is never synchronised inside the loop."""
    torch = torch_
    cases = (dc.short_case(17), dc.short_case(18)) if kind == "direct" else (dc.long_case(77), dc.long_case(78))
    assert np.array_equal(cases[0].lengths, cases[1].lengths)
    dev = [[torch.from_numpy(x).cuda() for x in (c.tid, c.pos, c.span)] for c in cases]
    rt, rs, re_ = cases[0].regions()
    R = len(rt)
    tables = [dc.guarded_table(torch, R, lead, dc.TAIL, side) for lead in dc.LEADS]
    eng = CoverageEngine(0)
    try:
        eng.set_contigs(cases[0].lengths)
        t0 = eng.timings()
        for step in range(32):
            k = step & 1
            lead = dc.LEADS[(step >> 1) & 1]
            table, at = tables[(step >> 1) & 1]
            eng.clear_reads()
            eng.add_reads(*dev[k])
            eng.compute_depth_stats_device(rt, rs, re_, at)
            host = dc.read_back(torch, table, side)
            dc.check(host, lead, R, cases[k].rows(), "step %d" % step)
            if kind == "recompute":     # (host-side counters: no synchronise)
                assert eng.fused_recomputes() > 0 and eng.fused_fallbacks() == 0, step
            else:
                assert (eng.fused_fallbacks(), eng.fused_recomputes()) == (0, 0), step
        d = delta(t0, eng.timings(), *PREP)
        assert d == ((32, 0, 32) if kind == "direct" else (0, 32, 32)), d
    finally:
        eng.close()


# ------------------------------------------------ 3. the benchmark's sequence at small size

@pytest.mark.parametrize("variant", ["fused", "unfused", "cigar"])
def test_benchmark_sequence(torch_, side, variant):
    """bench.py's step with the region-table exchange, small: resident tuples,
    two exchange tables of G slots of r_max rows, 2 + 8 steps that pass the
    same region array objects and write into the step's slot."""
    torch = torch_
    case = dc.short_case()
    R, G = case.R, 4
    r_max = R + 3
    tid, pos, span = (torch.from_numpy(x).cuda() for x in (case.tid, case.pos, case.span))
    xbufs = [dc.sentinel_table(torch, G * r_max, side) for _ in range(2)]
    rt, rs, re_ = case.regions()
    eng = CoverageEngine(0)
    try:
        eng.set_contigs(case.lengths)
        cig_off = cigar = None
        if variant == "cigar":
            cig_off, cigar = synth.device_cigars(torch, span, mean_ops=30, seed=3, batch_reads=10_000)
            torch.cuda.synchronize()
            eng.add_reads_cigar_device(tid, pos, cig_off, cigar)
        else:
            eng.add_reads(tid, pos, span)
        t0 = eng.timings()
        for k in range(2 + 8):
            i, slot = (k // G) & 1, k % G
            tbl = xbufs[i][slot * r_max:slot * r_max + R]
            assert tbl.data_ptr() == xbufs[i].data_ptr() + slot * r_max * ROW_BYTES
            if variant == "cigar":
                eng.clear_reads()
                eng.add_reads_cigar_device(tid, pos, cig_off, cigar)
            else:
                eng.invalidate()
            if variant == "unfused":
                eng.compute_depth()
                eng.region_stats_device(rt, rs, re_, tbl.data_ptr())
            else:
                eng.compute_depth_stats_device(rt, rs, re_, tbl.data_ptr())
                assert eng._rcache[0] is rt and eng._rcache[1] is rs and eng._rcache[2] is re_
        for i in range(2):
            host = dc.read_back(torch, xbufs[i], side)
            for slot in range(G):     # rows R .. r_max of every slot are the guard
                dc.check(host[slot * r_max:(slot + 1) * r_max], 0, R, case.rows(), (variant, i, slot))
        t1 = eng.timings()
        if variant == "cigar":
            assert eng.aligned_bases() == int(case.span.astype(np.int64).sum())
            assert t1["cigar_ms"] > 0
        else:
            assert delta(t0, t1, "direct_batches", "full_prepares") == (10, 0)
        assert delta(t0, t1, "fused_calls")[0] == (0 if variant == "unfused" else 10)
    finally:
        eng.close()


# ------------------------------------------------ 4. in-place region arrays

def test_region_arrays_rewritten_in_place(torch_, side):
    """The same three numpy objects with other contents: the engine reuses
    their pointers (CoverageEngine._region_args) and the library compares the
    contents, so the rows follow them: other starts / ends (restaged), a
    permutation (restaged), the same contents again (the staged set reused)."""
    torch = torch_
    case = dc.short_case()
    a = dc.tiling(np.random.default_rng(5), case.lengths, 7)
    b = dc.tiling(np.random.default_rng(6), case.lengths, 7)
    assert len(a[0]) == len(b[0]) and not np.array_equal(a[1], b[1])
    perm = np.random.default_rng(7).permutation(len(a[0]))
    rt, rs, re_ = (x.copy() for x in a)
    eng = CoverageEngine(0)
    try:
        load(eng, case)
        args = None
        for fresh in (False, True):      # on a reused index, then as the benchmark's fresh batches
            for k, new in enumerate((a, b, tuple(x[perm] for x in b), None)):
                if new is not None:
                    rt[:], rs[:], re_[:] = new
                if fresh:
                    eng.invalidate()
                before = eng.timings()["fused_calls"]
                run(torch, eng, side, case, dc.LEADS[k & 1], regs=(rt, rs, re_), what=(fresh, k))
                assert eng.timings()["fused_calls"] == before + 1
                assert eng._rcache[0] is rt and eng._rcache[1] is rs and eng._rcache[2] is re_
                assert args is None or eng._rcache[3] is args     # the cached C arguments, not new ones
                args = eng._rcache[3]
    finally:
        eng.close()


# ------------------------------------------------ 5. K3's histogram switch

@pytest.mark.parametrize("depth", dc.HIST_SWITCH_DEPTHS)
def test_k3_histogram_switch(torch_, side, depth):
    """Plain K3 with nbins = kLdsBins (the last LDS histogram), kLdsBins + 1
    and kLdsBins + 2 (the global one)."""
    case = dc.pile_case(depth)
    eng = CoverageEngine(0)
    try:
        load(eng, case)
        for lead in dc.LEADS:
            t0 = eng.timings()
            run(torch_, eng, side, case, lead, call="k3")
            assert delta(t0, eng.timings(), "stats_launches", "fused_calls") == (1, 0)
            assert eng.max_depth() == depth
    finally:
        eng.close()


def test_fused_histogram_switch(torch_, side):
    """The fused call's recompute at maximum depth kLdsBins - 1 (the device's
    histogram still holds it) and kLdsBins (handed to the host's K3)."""
    eng = CoverageEngine(0)
    try:
        for depth in (fm.K_LDS_BINS - 1, fm.K_LDS_BINS):
            case = dc.long_case(pile=depth)
            eng.set_contigs(case.lengths)
            eng.add_reads(case.tid, case.pos, case.span)
            for lead in dc.LEADS:
                run(torch_, eng, side, case, lead, what=depth)
                assert eng.max_depth() == depth
                if depth < fm.K_LDS_BINS:
                    assert eng.fused_recomputes() > 0 and eng.fused_fallbacks() == 0
                else:
                    assert eng.fused_recomputes() == 0 and eng.fused_fallbacks() > 0
    finally:
        eng.close()


# ------------------------------------------------ 6. K3's region batching

def _need_memory(torch):
    free, _ = torch.cuda.mem_get_info()
    if free < 4 << 30:
        pytest.skip("K3's value histogram of this case is about 1 GiB; the device reports %.1f GiB free"
                    % (free / 2.0**30))


def test_k3_region_batches_plain(torch_, side):
    """9003 regions at depth 65536: three batches of at most 4095 regions,
    rows exact in input order (d_out_final + r0)."""
    _need_memory(torch_)
    case = dc.batch_plain_case()
    eng = CoverageEngine(0)
    try:
        load(eng, case)
        for lead in dc.LEADS:
            t0 = eng.timings()
            run(torch_, eng, side, case, lead, call="k3")
            assert delta(t0, eng.timings(), "stats_launches")[0] == 3      # one region_seg_kernel launch per batch
        assert eng.max_depth() == dc.BATCH_DEPTH
    finally:
        eng.close()


@pytest.mark.parametrize("direct", [True, False])
def test_k3_region_batches_fallback(torch_, side, direct):
    """5001 flagged regions at depth 65536: the fused call hands them to the
    host's K3, which takes them in two batches and scatters the rows through
    out_rows + r0."""
    _need_memory(torch_)
    case = dc.batch_fallback_case()
    eng = CoverageEngine(0)
    try:
        load(eng, case, direct)
        for lead in dc.LEADS:
            eng.invalidate()
            t0 = eng.timings()
            run(torch_, eng, side, case, lead)
            assert (eng.fused_fallbacks(), eng.fused_recomputes()) == (case.R, 0) == (5001, 0)
            assert eng.max_depth() == dc.BATCH_DEPTH
            d = delta(t0, eng.timings(), "direct_batches", "full_prepares", "fused_calls", "stats_launches")
            assert d == ((1, 0) if direct else (0, 1)) + (1, 1 + 2), d      # K3b, then two K3 batches
    finally:
        eng.close()


# ------------------------------------------------ 7. errors leave the table alone

def test_errors_leave_the_table_alone(torch_, side):
    torch = torch_
    case = dc.short_case()
    rt, rs, re_ = case.regions()
    eng = CoverageEngine(0)
    try:
        load(eng, case)
        table, at = dc.guarded_table(torch, case.R, 3, dc.TAIL, side)
        with pytest.raises(MetacovError) as ei:
            eng.region_stats_device(rt, rs, re_, at)          # before any compute_depth
        assert ei.value.code == MC_E_STATE
        bad_tid = rt.copy()
        bad_tid[1] = len(case.lengths)
        bad_end = re_.copy()
        bad_end[2] = rs[2] - 1
        for fused in (True, False):
            call = eng.compute_depth_stats_device if fused else eng.region_stats_device
            if not fused:
                eng.compute_depth()
            with pytest.raises(MetacovError) as ei:
                call(rt, rs, re_, 0)                          # R > 0, null pointer
            assert ei.value.code == MC_E_INVALID
            with pytest.raises(MetacovError) as ei:
                call(bad_tid, rs, re_, at)
            assert ei.value.code == MC_E_INVALID
            with pytest.raises(MetacovError) as ei:
                call(rt, rs, bad_end, at)
            assert ei.value.code == MC_E_INVALID
        host = dc.read_back(torch, table, side)
        assert (host == dc.SENTINEL).all()
        # and the engine still works: the same table, now written
        eng.compute_depth_stats_device(rt, rs, re_, at)
        dc.check(dc.read_back(torch, table, side), 3, case.R, case.rows(), "after the errors")
    finally:
        eng.close()
