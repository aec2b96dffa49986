"""TEST INFRASTRUCTURE ONLY: the cases and the harness of the device-output
statistics tests (tests/test_gpu_device_rows.py on the GPU,
tests/test_device_rows_model.py for the cases' preconditions on the CPU).

compute_depth_stats_device and region_stats_device write their rows to a
caller's device pointer and return without a stream synchronise (the fused
call returns on a stamp in mapped host memory).  The harness gives them a
table with guard rows on both sides, reads it back on a stream of the test's
own without touching the engine's, and compares every field with the oracle.

A case is the batch (lengths, tid, pos, span) and a region list; its oracle
rows are computed once per process and shared.
"""
import os
import re

import numpy as np

from oracle import coracle
from tests import fused_model as fm

SENTINEL = -1
ROW_WORDS = 9                # int64 words of one mc_region_stat (72 bytes)
LEADS = (2, 3)               # row `lead` starts at byte 72 * lead: 16-byte aligned (even) and not (odd)
TAIL = 2

SHORT_LENGTHS = (60_000, 90_000, 30_000)
EMPTY_CONTIG = 500           # the read-less contig short_case(empty=True) appends
LONG_CONTIGS = 12
PILE_CONTIG = 1000           # the contig long_case(pile=D) appends for its pile
PILE_POS, PILE_SPAN = 100, 50


class Case:
    """A batch and a region list."""

    def __init__(self, lengths, tid, pos, span, rt, rs, re_):
        self.lengths = np.asarray(lengths, np.int64)
        self.tid, self.pos, self.span = (np.ascontiguousarray(x, np.int32) for x in (tid, pos, span))
        self.rt = np.ascontiguousarray(rt, np.int32)
        self.rs = np.ascontiguousarray(rs, np.int64)
        self.re = np.ascontiguousarray(re_, np.int64)
        self._depth = self._rows = None

    @property
    def R(self):
        return len(self.rt)

    def regions(self):
        """Fresh copies of the region arrays (a test may rewrite them in place)."""
        return self.rt.copy(), self.rs.copy(), self.re.copy()

    def depth(self):
        """(depth vector, extents, offsets) of the oracle."""
        if self._depth is None:
            self._depth = coracle.depth(self.lengths, self.tid, self.pos, self.span)
        return self._depth

    def rows(self):
        """The oracle's rows of the case's own regions (computed once; do not modify)."""
        if self._rows is None:
            self._rows = self.rows_of(self.rt, self.rs, self.re)
            self._rows.setflags(write=False)
        return self._rows

    def rows_of(self, rt, rs, re_):
        d, ext, coff = self.depth()
        return coracle.region_stats(d, ext, coff, rt, rs, re_)

    def with_regions(self, rt, rs, re_):
        """The same batch (and its cached depth) under other regions."""
        c = Case(self.lengths, self.tid, self.pos, self.span, rt, rs, re_)
        c._depth = self._depth
        return c


def whole_contigs(lengths):
    n = len(lengths)
    return np.arange(n, dtype=np.int32), np.zeros(n, np.int64), np.asarray(lengths, np.int64).copy()


def make_case(lengths, n, span_rng, seed, overhang=True):
    """Uniform sorted reads (as test_gpu_parity.make_case)."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, np.int64)
    live = np.nonzero(lengths > 0)[0]
    tid = rng.choice(live, size=n).astype(np.int32)
    pos = (rng.random(n) * lengths[tid]).astype(np.int32)
    span = rng.integers(span_rng[0], span_rng[1] + 1, size=n).astype(np.int32)
    if not overhang:
        span = np.minimum(span, (lengths[tid] - pos)).astype(np.int32)
    o = np.lexsort((pos, tid))
    return lengths, tid[o], pos[o], span[o]


_CACHE = {}


def _once(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def short_case(seed=17, empty=False):
    """Short reads over three contigs, whole-contig regions: the direct path
    (or, with set_direct_prepare(False), the full prepare).  No read runs
    past its contig (such a batch leaves the direct path).  Depth ~25, so
    every window base is 0 and no region is recomputed.  empty: a fourth
    contig without reads."""
    def fn():
        lengths, tid, pos, span = make_case(SHORT_LENGTHS, 30_000, (1, 300), seed, overhang=False)
        if empty:
            lengths = np.concatenate([lengths, [EMPTY_CONTIG]])
        return Case(lengths, tid, pos, span, *whole_contigs(lengths))
    return _once(("short", seed, empty), fn)


def long_case(seed=77, pile=None):
    """Device recompute: 12 contigs of 20-40 kbp (fixed) under ~80 k lognormal
    ~8 kbp reads drawn by `seed` (test_fused_device_recompute in miniature):
    long reads switch the device recompute on, and the end ramps push the
    whole-contig regions' ranks out of their windows.  pile=D: one more contig
    of 1000 positions that holds only D reads on one spot, so the batch's
    maximum depth is exactly D when D exceeds the other contigs' depth."""
    def fn():
        lengths = np.random.default_rng(7).integers(20_000, 40_001, size=LONG_CONTIGS).astype(np.int64)
        w = np.minimum(np.random.default_rng(8).lognormal(0, 1.0, size=LONG_CONTIGS), 4.0)
        rng = np.random.default_rng(seed)
        n = 80_000
        tid = np.sort(rng.choice(LONG_CONTIGS, size=n, p=w / w.sum())).astype(np.int32)
        span = np.minimum(rng.lognormal(np.log(8000), 0.4, size=n).astype(np.int64), lengths[tid]).astype(np.int32)
        pos = (rng.random(n) * (lengths[tid] - span + 1)).astype(np.int32)
        if pile is not None:
            lengths = np.concatenate([lengths, [PILE_CONTIG]])
            tid = np.concatenate([tid, np.full(pile, LONG_CONTIGS, np.int32)])
            pos = np.concatenate([pos, np.full(pile, PILE_POS, np.int32)])
            span = np.concatenate([span, np.full(pile, PILE_SPAN, np.int32)])
        o = np.lexsort((pos, tid))
        return Case(lengths, tid[o], pos[o], span[o], *whole_contigs(lengths))
    return _once(("long", seed, pile), fn)


def slot_case(variant):
    """fused_model's slot set: K_FB_SLOTS + 1 flagged regions, one more than
    the device recompute takes, so the host's K3 recomputes them all."""
    def fn():
        b = fm.built("slot", variant)
        return Case(b.lengths, b.tid, b.pos, b.span, b.rtid, b.rs, b.re)
    return _once(("slot", variant), fn)


def tiling(rng, lengths, pieces):
    """Non-overlapping regions that tile every contig and run 37 past its
    end, in a random order (as test_gpu_parity._tiling)."""
    rt, rs, re_ = [], [], []
    for t, L in enumerate(lengths):
        cuts = np.sort(rng.integers(0, L + 1, size=pieces))
        edges = np.concatenate([[0], cuts, [L + 37]])
        for a, b in zip(edges[:-1], edges[1:]):
            rt.append(t)
            rs.append(a)
            re_.append(b)
    o = rng.permutation(len(rt))
    return np.array(rt, np.int32)[o], np.array(rs, np.int64)[o], np.array(re_, np.int64)[o]


def shape_case(name):
    """The short batch (with its empty contig) under other region shapes."""
    def fn():
        base = short_case(empty=True)
        L = base.lengths
        if name == "overlap":       # not fusable: K2 then K3
            regs = ([0, 0, 1, 1, 2, 3], [0, 10_000, 5, 5, 100, 0], [30_000, 50_000, 80_000, 80_000, 30_400, 500])
        elif name == "r1":
            regs = ([1], [1_000], [77_001])
        elif name == "r5":          # not a multiple of K3b's four waves
            regs = ([2, 0, 1, 0, 3], [7, 0, 45_000, 30_001, 1], [29_990, 30_001, 90_100, 60_000, 499])
        elif name == "r1000":       # one-position regions, every 61st position of contig 1, permuted
            p = np.random.default_rng(3).permutation(1000).astype(np.int64) * 61 + 13
            regs = (np.ones(1000, np.int32), p, p + 1)
        elif name == "zeros":       # wholly past the extent, and the contig without reads: n > 0, all zeros
            regs = ([0, 3, 1, 3, 2], [L[0] + 1000, 0, L[1] + 5000, 300, L[2] + 400],
                    [L[0] + 1100, 200, L[1] + 5001, 900, L[2] + 4500])
        else:
            raise KeyError(name)
        return base.with_regions(*regs)
    return _once(("shape", name), fn)


SHAPES = ("overlap", "r1", "r5", "r1000", "zeros")


# ---- K3's histogram switch and region batching

HIST_SWITCH_DEPTHS = (fm.K_LDS_BINS - 1, fm.K_LDS_BINS, fm.K_LDS_BINS + 1)


def pile_case(depth, length=1000, pos=PILE_POS, span=PILE_SPAN, regions=None):
    """`depth` reads on one spot of one contig."""
    def fn():
        regs = regions
        if regs is None:    # the whole contig, one that cuts the pile, one that misses it, one past the extent
            regs = ([0, 0, 0, 0], [0, pos + span // 2, pos + span + 50, 2 * length],
                    [length, pos + 300, length - 100, 2 * length + 100])
        return Case([length], np.zeros(depth, np.int32), np.full(depth, pos, np.int32),
                    np.full(depth, span, np.int32), *regs)
    return fn() if regions is not None else _once(("pile", depth, length, pos, span), fn)


BATCH_DEPTH = 65536          # the piles of the two batching cases: nbins = 65537, rb = 4095


def batch_plain_case():
    """K3's region batching, plain: 9000 overlapping regions [7 r, 7 r + 1 +
    r % 50) in a permuted order and three regions over the pile, one in each
    third of the order; at depth 65536 K3 takes them in three batches."""
    def fn():
        r = np.arange(9000, dtype=np.int64)
        rs, re_ = 7 * r, 7 * r + 1 + r % 50
        o = np.random.default_rng(6).permutation(9000)
        rs, re_ = list(rs[o]), list(re_[o])
        for at, (a, b) in ((8000, (50, 400)), (4500, (110, 130)), (1000, (0, 70_000))):   # (back to front)
            rs.insert(at, a)
            re_.insert(at, b)
        regs = (np.zeros(len(rs), np.int32), np.array(rs, np.int64), np.array(re_, np.int64))
        return pile_case(BATCH_DEPTH, 70_000, 100, 40, regions=regs)
    return _once("batch_plain", fn)


def batch_fallback_case():
    """K3's region batching through the fused call's host fallback: every
    region lies below its window (the pile lifts the contig's window base to
    689; the depth is 0 nearly everywhere), 5001 flagged regions exceed the
    device recompute's slots and the depth its histogram, so the host's K3
    recomputes them in two batches and scatters the rows through out_rows."""
    def fn():
        k = np.arange(5000, dtype=np.int64)
        regs = (np.zeros(5001, np.int32), np.concatenate([[0], 10_000 + 2 * k]),
                np.concatenate([[10_000], 10_002 + 2 * k]))
        return pile_case(BATCH_DEPTH, 20_000, 100, 400, regions=regs)
    return _once("batch_fallback", fn)


def source_max_hist():
    """K3's histogram budget in bins (region_stats_impl's max_hist), as
    engine.hip defines it."""
    e = open(os.path.join(fm.CSRC, "engine.hip")).read()
    m = re.search(r"const int64_t max_hist = int64_t\(1\) << (\d+);", e)
    assert m and re.search(r"std::min<int64_t>\(R, max_hist / nbins\)", e), "region_stats_impl's batching changed"
    return 1 << int(m.group(1))


def region_batch(max_depth):
    """Regions per K3 batch at this maximum depth (rb of region_stats_impl)."""
    return max(1, source_max_hist() // (max_depth + 1))


def model_flags(case, variant):
    """K3b's flag per region of the case, by fused_model: the window bases
    of the prepare path `variant` ("full" or "direct") and classify()."""
    d, ext, coff = case.depth()
    if variant == "direct":
        assert np.array_equal(ext, case.lengths)
        base = fm.window_base_direct(case.lengths, case.tid, case.span)
    else:
        base = fm.window_base_full(ext, case.tid, case.span)
    flags = np.zeros(case.R, bool)
    for r in range(case.R):
        t = int(case.rt[r])
        x = int(ext[t])
        a, e = min(int(case.rs[r]), x), min(int(case.re[r]), x)
        zx = int(case.re[r] - case.rs[r]) - (e - a)
        flags[r] = fm.classify(d[coff[t]:coff[t] + x], a, e, int(base[t]), zx)["flag"]
    return base, flags


# ---- the harness (the torch module is passed in: this file imports without it)

def sentinel_table(torch, rows, side):
    """An int64 device table [rows, 9] filled with the sentinel on the stream
    `side`, which is synchronised before this returns: the fill is ordered
    before whatever the engine writes, without touching the engine's stream.
    The pinned host buffer read_back() copies into is made here too, so that
    nothing but the copy lies between an engine call's return and the read."""
    with torch.cuda.stream(side):
        table = torch.full((rows, ROW_WORDS), SENTINEL, dtype=torch.int64, device="cuda")
    table.host_copy = torch.empty(table.shape, dtype=table.dtype, pin_memory=True)
    side.synchronize()
    return table


def guarded_table(torch, R, lead, tail, side):
    """A sentinel table with `lead` guard rows before the R rows of the
    destination and `tail` after them.  Returns the table and the address of
    row `lead`."""
    table = sentinel_table(torch, lead + R + tail, side)
    return table, table.data_ptr() + lead * ROW_WORDS * 8


def read_back(torch, table, side):
    """The table (of sentinel_table) on the host, copied on `side` and waiting
    for `side` only: no device-wide synchronise, nothing on the engine's
    stream."""
    with torch.cuda.stream(side):
        table.host_copy.copy_(table, non_blocking=True)
    side.synchronize()
    return table.host_copy.numpy().copy()


def check(table_host, lead, R, want, what=""):
    """Rows [lead, lead + R) equal `want` field by field; every other row is
    still the sentinel."""
    from metacov_amd.engine import REGION_STAT_DTYPE
    assert table_host.shape[1] == ROW_WORDS and len(want) == R
    got = np.ascontiguousarray(table_host[lead:lead + R]).view(REGION_STAT_DTYPE).reshape(-1)
    for f in want.dtype.names:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, (what, f, [(int(r), int(got[f][r]), int(want[f][r])) for r in bad[:5]], len(bad))
    guards = np.concatenate([table_host[:lead], table_host[lead + R:]])
    bad = np.nonzero((guards != SENTINEL).any(axis=1))[0]
    assert len(bad) == 0, (what, "guard rows overwritten", [int(r) if r < lead else int(r) + R for r in bad[:5]])
