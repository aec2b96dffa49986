"""The fused statistics window on the GPU at its edges: values at base - 1,
base, base + 863 and base + 864, ranks on the first and last rank the window
holds, runs across the edges inside one int4, many tiny regions, a region
across a chunk boundary, the 512-slot hand-over and the recompute state
across calls.  Every row and the depth are compared with the oracle, and the
number of recomputed regions and the path that recomputed them with the model
(tests/fused_model.py), on the full prepare, on the direct path and with long
reads.  tests/test_fused_model.py checks the cases' preconditions on the CPU.

Run on an MI355X:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest

from oracle import coracle
from metacov_amd.engine import CoverageEngine
from tests import fused_model as fm

pytestmark = pytest.mark.gpu

_REF = {}


def reference(b):
    """The oracle's depth and rows and the model's flags of a built case set
    (computed once, shared by the tests)."""
    if id(b) not in _REF:
        d, ext, coff = coracle.depth(b.lengths, b.tid, b.pos, b.span)
        rows = coracle.region_stats(d, ext, coff, b.rtid, b.rs, b.re)
        flags = np.array([c["flag"] for c in fm.model_rows(b)[1]], bool)
        _REF[id(b)] = (b, d, ext, coff, rows, flags)
    return _REF[id(b)][1:]


def engine_for(b, variant, lib_built):
    e = CoverageEngine(0)
    if variant == "full":
        e.set_direct_prepare(False)
    e.set_contigs(b.lengths)
    e.add_reads(b.tid, b.pos, b.span)
    return e


def check_prepare(e, variant, batches=1):
    t = e.timings()
    if variant == "direct":
        assert t["direct_batches"] == batches and t["full_prepares"] == 0
    else:   # (long reads: the direct attempt is refused and redone on the full prepare)
        assert t["direct_batches"] == 0 and t["full_prepares"] == batches


def call(e, b, device_on, sel=None):
    """One fused call on the regions `sel` of b: rows against the oracle, the
    recomputed regions and their path against the model.  device_on: the
    device recompute runs in this call.  Returns it for the next call."""
    d, ext, coff, rows, flags = reference(b)
    sel = np.arange(len(b.rtid)) if sel is None else np.asarray(sel)
    before = e.timings()["fused_calls"]
    got = e.compute_depth_stats(b.rtid[sel], b.rs[sel], b.re[sel])
    assert e.timings()["fused_calls"] == before + 1, "the fused path did not run"
    for f in rows.dtype.names:
        bad = np.nonzero(got[f] != rows[f][sel])[0]
        assert len(bad) == 0, (f, [(int(sel[r]), b.items[sel[r]].tag if b.items[sel[r]] else None,
                                    int(got[f][r]), int(rows[f][sel[r]])) for r in bad[:5]])
    count = int(flags[sel].sum())
    assert e.fused_fallbacks() + e.fused_recomputes() == count
    assert (e.fused_fallbacks(), e.fused_recomputes()) == fm.recompute_path(count, device_on, e.max_depth())
    return b.long_read or count > 0


def check_depth(e, b):
    d, ext, coff, rows, flags = reference(b)
    for t in range(len(b.lengths)):
        assert np.array_equal(e.depth(t, 0, int(ext[t])), d[coff[t]:coff[t] + ext[t]]), "contig %d" % t


@pytest.mark.parametrize("variant", fm.VARIANTS)
@pytest.mark.parametrize("name", ["rank_edges", "value_edges", "compose", "tiny", "chunk"])
def test_case_set(lib_built, name, variant):
    """Two identical calls on a fresh engine: short reads have the first call's
    flagged regions recomputed by the host's K3 and the second's on the
    device; long reads both on the device."""
    b = fm.built(name, variant)
    flags = reference(b)[4]
    assert 0 < flags.sum() <= fm.K_FB_SLOTS
    e = engine_for(b, variant, lib_built)
    try:
        on = call(e, b, b.long_read)
        check_prepare(e, variant)
        check_depth(e, b)
        assert on
        assert (e.fused_fallbacks() > 0) == (variant != "long")
        call(e, b, on)
        assert e.fused_recomputes() == flags.sum() and e.fused_fallbacks() == 0
        check_prepare(e, variant)
        check_depth(e, b)
    finally:
        e.close()


@pytest.mark.parametrize("variant", fm.VARIANTS)
def test_slot_edge(lib_built, variant):
    """512 flagged regions are recomputed on the device, 513 by the host's K3."""
    b = fm.built("slot", variant)
    flags = reference(b)[4]
    n = fm.K_FB_SLOTS
    assert flags.sum() == n + 1 and flags[:n + 1].all()
    s512 = np.concatenate([np.arange(n), np.arange(n + 1, len(flags))])
    e = engine_for(b, variant, lib_built)
    try:
        on = call(e, b, b.long_read, s512)
        on = call(e, b, on, s512)
        assert (e.fused_fallbacks(), e.fused_recomputes()) == (0, n)
        on = call(e, b, on)
        assert (e.fused_fallbacks(), e.fused_recomputes()) == (n + 1, 0)
        check_depth(e, b)
        on = call(e, b, on, s512)
        assert (e.fused_fallbacks(), e.fused_recomputes()) == (0, n)
        on = call(e, b, on, s512[::-1])
        assert (e.fused_fallbacks(), e.fused_recomputes()) == (0, n)
    finally:
        e.close()


@pytest.mark.parametrize("variant", fm.VARIANTS)
def test_stale_recompute_state(lib_built, variant):
    """Flagged sets A, a disjoint B, A again, then no flagged region, then A:
    nothing of one call's recompute (its list, histograms, accumulators, the
    switch to the device) leaks into the next."""
    b = fm.built("rank_edges", variant)
    flags = reference(b)[4]
    hot, cold = np.nonzero(flags)[0], np.nonzero(~flags)[0]
    sa = np.sort(np.concatenate([hot[0::2], cold[0::2]]))
    sb = np.sort(np.concatenate([hot[1::2], cold[1::2]]))
    assert len(hot) >= 8 and not set(sa) & set(sb)
    e = engine_for(b, variant, lib_built)
    try:
        on = b.long_read
        for sel in (sa, sb, sa, cold, sa, sb):
            on = call(e, b, on, sel)
        assert e.fused_recomputes() == flags[sb].sum()
        check_depth(e, b)
    finally:
        e.close()


@pytest.mark.parametrize("variant", fm.VARIANTS)
@pytest.mark.parametrize("name", ["rank_edges", "compose"])
def test_new_batch_same_layout(lib_built, name, variant):
    """A second batch of another depth over the same contigs and regions: the
    staged regions stand and only the window bases follow (on the full
    prepare: window_bases_kernel, which must place the windows where the host
    would, also for compose's exact half and its reads past a contig's
    length; on the direct path: the new probe)."""
    b1 = fm.built(name, variant)
    b2 = fm.built(name, "direct" if variant == "direct" else "full", long_read=b1.long_read, depth=2200)
    assert np.array_equal(b1.lengths, b2.lengths) and np.array_equal(b1.extent, b2.extent)
    assert np.array_equal(b1.rs, b2.rs) and np.array_equal(b1.re, b2.re)
    assert not np.array_equal(b1.base, b2.base) and (b2.base[[0, 2]] > 0).all()
    e = engine_for(b1, variant, lib_built)
    try:
        on = call(e, b1, b1.long_read)
        e.clear_reads()
        e.add_reads(b2.tid, b2.pos, b2.span)
        on = call(e, b2, on)
        check_prepare(e, variant, 2)
        check_depth(e, b2)
        call(e, b2, on)
    finally:
        e.close()
