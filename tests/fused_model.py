"""TEST INFRASTRUCTURE ONLY: a numpy model of the fused statistics window
(csrc/kernels.h: hist_int4, final_wave_row, direct_window_base, probe_kernel,
window_bases_kernel; csrc/engine.hip: depth_stats_once, depth_stats_launch)
and the case builders the CPU and GPU window tests share.

K2 folds each region's values into a histogram of kHistBins values that
starts at the region's window base; values outside it go to an overflow
accumulator and the count below the window.  K3b composes the row from the
window, the accumulator and the zeros past the contig extent (`zx`), and
flags the regions whose median / quartile ranks leave the window; those are
recomputed exactly.  The model predicts, for a batch and a region list, every
window base, every flag and every row K3b writes before the recompute, so a
test can place values and ranks exactly on the window's edges and assert how
many regions are recomputed.

Everything is integer and exact.  The constants mirror kernels.h / engine.hip
(test_fused_model.py::test_constants_match_source reads them from there).
"""
import math
import os
import re

import numpy as np

K_HIST_BINS = 864            # HistCfg<false>::kBins (MC_HIST_COPIES == 2)
K_WIN_BELOW = 648            # MC_WIN_BELOW = 3 * kHistBins / 4
K_FB_SLOTS = 512             # kFbSlots
K_LDS_BINS = 16384           # kLdsBins
K_PROBE_STRIDE = 256         # kProbeStride
K_PROBE_SPAN_EVERY = 4       # kProbeSpanEvery
K_PROBE_MEAN_BLOCKS = 64     # kProbeMeanBlocks
K_BLOCK = 256                # kBlock
K_TILE_W = 4096              # MC_TILE_W
K_SHORT_MAX = 4096           # MC_RING - MC_TILE_W: longer reads take the long-read K2
K_TILES_PER_CHUNK = 8        # MC_TILES_PER_CHUNK
K_TILES_PER_CHUNK_LONG = 16  # MC_TILES_PER_CHUNK_LONG
K_MIN_CHUNKS = 2048          # MC_MIN_CHUNKS
INT_MAX = 0x7fffffff

ROW_FIELDS = ("n", "sum", "sumsq", "min", "max", "med_lo", "med_hi", "q23_sum", "q23_cnt")
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metacov_amd", "csrc")


def source_constants():
    """The same constants as the sources define them (for the test that
    keeps this model's copies honest)."""
    k = open(os.path.join(CSRC, "kernels.h")).read()
    e = open(os.path.join(CSRC, "engine.hip")).read()

    def num(text, pat):
        return int(re.search(pat, text).group(1))

    copies = num(k, r"#define MC_HIST_COPIES (\d+)")
    bins = {int(a): int(b) for a, b in re.findall(r"MC_HIST_COPIES == (\d+) \? (\d+)", k)}[copies]
    assert re.search(r"#define MC_HIST_COPIES_LONG MC_HIST_COPIES\b", k)
    assert re.search(r"#define MC_WIN_BELOW \(3 \* kHistBins / 4\)", e)
    assert re.search(r"#define MC_RING \(2 \* MC_TILE_W\)", k)
    tile = num(k, r"#define MC_TILE_W (\d+)")
    return {
        "K_HIST_BINS": bins,
        "K_WIN_BELOW": 3 * bins // 4,
        "K_FB_SLOTS": num(k, r"constexpr int kFbSlots = (\d+);"),
        "K_LDS_BINS": num(k, r"constexpr int kLdsBins = (\d+);"),
        "K_PROBE_STRIDE": 1 << num(k, r"constexpr int kProbeShift = (\d+);"),
        "K_PROBE_SPAN_EVERY": num(k, r"constexpr int kProbeSpanEvery = (\d+);"),
        "K_PROBE_MEAN_BLOCKS": num(k, r"constexpr unsigned kProbeMeanBlocks = (\d+);"),
        "K_BLOCK": num(k, r"constexpr int kBlock = (\d+);"),
        "K_TILE_W": tile,
        "K_SHORT_MAX": tile,
        "K_TILES_PER_CHUNK": num(k, r"#define MC_TILES_PER_CHUNK (\d+)"),
        "K_TILES_PER_CHUNK_LONG": num(k, r"#define MC_TILES_PER_CHUNK_LONG (\d+)"),
        "K_MIN_CHUNKS": num(e, r"#define MC_MIN_CHUNKS (\d+)"),
    }


# --------------------------------------------------------------- the model

class Params:
    """The window's rules; the defaults are the kernels'.  The mutants of
    test_fused_model.py change one field each."""

    def __init__(self, **kw):
        self.kwin = K_HIST_BINS          # hist_int4: d >= kWin is out of the window
        self.win_below = K_WIN_BELOW
        self.rounding = "llrint"         # window_base (host), window_bases_kernel, direct_window_base
        self.q_lo_le = False             # q_lo < win_lo  ->  q_lo <= win_lo
        self.q_hi_gt = False             # q_hi - 1 >= win_hi  ->  q_hi - 1 > win_hi
        self.min_rule = True             # base > 0 && zx > 0: the minimum is 0
        self.max_high_ge = False         # high > 0  ->  high >= 0
        self.zx_bin_always = False       # zx counted in bin 0 whatever the base
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


def llround(x):
    """C llround for x >= 0: halves away from zero."""
    f = math.floor(x)
    return int(f) + (1 if x - f >= 0.5 else 0)


def llrint(x):
    """C llrint in the default rounding mode: halves to even."""
    return int(round(x))


_ROUND = {"llround": llround, "llrint": llrint}


def reads_for_profile(d, max_span):
    """Sorted reads (pos, span) of one contig whose depth is exactly the
    integer profile d: position p starts d[p] - d[p-1] reads or ends that
    many, starts and ends are paired first in, first out, and a read that
    reaches max_span ends there and starts again at the same position.  Every
    read ends at or before len(d), so the depth is 0 at the contig end."""
    d = np.asarray(d, np.int64)
    assert d.ndim == 1 and (d >= 0).all()
    e = np.diff(np.concatenate(([0], d, [0])))
    idx = np.arange(len(d) + 1, dtype=np.int64)
    starts = np.repeat(idx, np.maximum(e, 0))
    ends = np.repeat(idx, np.maximum(-e, 0))
    pieces = (ends - starts + max_span - 1) // max_span
    first = np.cumsum(pieces) - pieces
    k = np.arange(int(pieces.sum()), dtype=np.int64) - np.repeat(first, pieces)
    pos = np.repeat(starts, pieces) + k * max_span
    span = np.minimum(max_span, np.repeat(ends, pieces) - pos)
    o = np.argsort(pos, kind="stable")
    return pos[o].astype(np.int32), span[o].astype(np.int32)


def window_base_full(extent, tid, span, params=None):
    """Every contig's window base on the full prepare: the host lambda
    window_base of depth_stats_once and window_bases_kernel, which a batch
    prepared over an already staged layout takes (a new batch, or a direct
    attempt redone on the full prepare).  The mean span over the whole batch,
    the contig's bases over its extent (its length, or its furthest read end)
    less one mean span if the extent exceeds two, llrint, win_below below it,
    clamped at 0."""
    p = params or Params()
    rnd = _ROUND[p.rounding]
    n = len(tid)
    mean = float(int(span.astype(np.int64).sum())) / float(n) if n else 0.0
    cb = np.zeros(len(extent), np.int64)
    np.add.at(cb, tid, span.astype(np.int64))
    out = np.zeros(len(extent), np.int64)
    for t, x in enumerate(extent):
        ext = float(x)
        body = ext - mean if ext > 2.0 * mean else ext
        est = float(cb[t]) / body if ext > 0 else 0.0
        out[t] = max(0, rnd(est) - p.win_below)
    return out


def window_base_direct(lengths, tid, span, params=None):
    """Every contig's window base on the direct path (direct_window_base from
    probe_kernel's samples): one sample every kProbeStride reads; the contig's
    reads ~ its samples x the stride; the mean of the spans of every
    kProbeSpanEvery-th sample, from the workgroups the probe takes them from;
    the contig length for the extent (a read past it sends the batch to the
    full prepare); llrint."""
    p = params or Params()
    rnd = _ROUND[p.rounding]
    n = len(tid)
    m = (n + K_PROBE_STRIDE - 1) // K_PROBE_STRIDE
    j = np.arange(m, dtype=np.int64)
    at = j * K_PROBE_STRIDE
    stid = tid[at]
    grid = max(1, (m + K_BLOCK - 1) // K_BLOCK)
    every = max(1, grid // K_PROBE_MEAN_BLOCKS)
    sel = (j % K_PROBE_SPAN_EVERY == 0) & ((j // K_BLOCK) % every == 0)
    s = span[at[sel]].astype(np.int64)
    s = s[s >= 0]
    ssum, scnt = int(s.sum()), len(s)
    out = np.zeros(len(lengths), np.int64)
    for t, x in enumerate(lengths):
        ns = int(np.searchsorted(stid, t + 1, "left") - np.searchsorted(stid, t, "left"))
        if ns <= 0 or scnt == 0:
            continue
        mean = float(ssum) / float(scnt)
        bases = float(ns) * float(K_PROBE_STRIDE) * mean
        ext = float(x)
        body = ext - mean if ext > 2.0 * mean else ext
        est = bases / body if ext > 0 else 0.0
        out[t] = max(0, rnd(est) - p.win_below)
    return out


def chunk_width(extent, long_hint=False):
    """K2's chunk width for a layout (set_layout): chunks are halved, down to
    the ring's two tiles, while there would be fewer than MC_MIN_CHUNKS."""
    off = sum((int(x) + 63) // 64 * 64 for x in extent)
    tiles = max(1, (off + K_TILE_W - 1) // K_TILE_W)
    tpc = K_TILES_PER_CHUNK_LONG if long_hint else K_TILES_PER_CHUNK
    while tpc // 2 >= 2 and tiles // tpc < K_MIN_CHUNKS:
        tpc //= 2
    return tpc * K_TILE_W


def contig_offsets(extent):
    """The engine's global layout: contigs start at multiples of 64."""
    off = np.zeros(len(extent) + 1, np.int64)
    off[1:] = np.cumsum([(int(x) + 63) // 64 * 64 for x in extent])
    return off


def classify(depth, gs, ge, base, zx, params=None):
    """One region's row as K3b composes it.  depth: the contig's depth
    vector; [gs, ge): the region clipped to the extent; zx: its positions past
    the extent.  Returns the counts below / inside / above the window, the
    ranks, `flag` (the region is recomputed) and `row` (what final_wave_row
    writes; only meaningful to the caller when flag is False)."""
    p = params or Params()
    v = np.asarray(depth[gs:ge], np.int64)
    n = len(v) + zx
    rel = v - base
    inside = (rel >= 0) & (rel < p.kwin)
    below = v < base
    out = ~inside
    zx_bin = zx if (base == 0 or p.zx_bin_always) else 0
    low = int(below.sum()) + (0 if base == 0 else zx)
    hist = np.bincount(rel[inside], minlength=p.kwin).astype(np.int64)
    hist[0] += zx_bin
    in_hist = int(hist.sum())
    r_lo, r_hi = (n - 1) // 2, n // 2
    q_lo, q_hi = n // 4, n - n // 4
    e = low + np.cumsum(hist)
    cum = e - hist
    vals = base + np.arange(p.kwin, dtype=np.int64)
    occ = hist > 0
    med_lo = med_hi = -1
    k = np.nonzero(occ & (cum <= r_lo) & (r_lo < e))[0]
    if len(k):
        med_lo = int(vals[k[0]])
    k = np.nonzero(occ & (cum <= r_hi) & (r_hi < e))[0]
    if len(k):
        med_hi = int(vals[k[0]])
    ov = np.minimum(e, q_hi) - np.maximum(cum, q_lo)
    qsum = int((np.maximum(ov, 0) * vals)[occ].sum())
    s1 = int((hist * vals).sum())
    s2 = int((hist * vals * vals).sum())
    lmin = int(np.nonzero(occ)[0][0]) if in_hist else INT_MAX
    lmax = int(np.nonzero(occ)[0][-1]) if in_hist else -1
    win_lo, win_hi = low, low + in_hist
    t_q_lo = q_lo <= win_lo if p.q_lo_le else q_lo < win_lo
    t_q_hi = q_hi - 1 > win_hi if p.q_hi_gt else q_hi - 1 >= win_hi
    flag = n > 0 and (r_lo < win_lo or r_hi >= win_hi or t_q_lo or t_q_hi)
    # the overflow accumulator: every value outside the window (RegionAcc)
    vo = v[out]
    a_sum = int(vo.sum())
    a_sq = int((vo * vo).sum())
    a_min = int(vo.min()) if len(vo) else INT_MAX
    a_max = int(vo.max()) if len(vo) else 0
    high = n - win_hi
    row = dict.fromkeys(ROW_FIELDS, 0)
    if n > 0:
        row["n"] = n
        row["sum"] = s1 + a_sum
        row["sumsq"] = s2 + a_sq
        if low > 0:
            m = a_min
            if p.min_rule and base > 0 and zx > 0:
                m = 0
            row["min"] = m
        else:
            row["min"] = base + lmin if in_hist > 0 else a_min
        above = high >= 0 if p.max_high_ge else high > 0
        row["max"] = max(0, a_max if above else (base + lmax if in_hist > 0 else a_max))
        row["med_lo"] = max(0, med_lo)
        row["med_hi"] = max(0, med_hi)
        row["q23_sum"] = qsum
        row["q23_cnt"] = q_hi - q_lo
    return {"n": n, "zx": zx, "low": low, "in_hist": in_hist, "high": high, "win_lo": win_lo, "win_hi": win_hi,
            "r_lo": r_lo, "r_hi": r_hi, "q_lo": q_lo, "q_hi": q_hi,
            "terms": (n > 0 and r_lo < win_lo, n > 0 and r_hi >= win_hi, n > 0 and t_q_lo, n > 0 and t_q_hi),
            "flag": bool(flag), "row": row}


def recompute_path(count, device_on, max_depth=0):
    """(fused_fallbacks, fused_recomputes) of a call that flags `count`
    regions.  device_on: the device recompute runs in this call (long reads,
    or the previous call flagged a region); it takes at most kFbSlots regions
    of depth below kLdsBins, the host's K3 the rest."""
    if device_on and count <= K_FB_SLOTS and max_depth < K_LDS_BINS:
        return 0, count
    return count, 0


# ------------------------------------------------------------ case builders
#
# A case set is a list of contigs.  A contig ramps up to a plateau of depth D,
# then carries one or more segments of items, then ramps down to 0.  An item
# is a cell (one region), a pad (no region) or the segment's bump (below); a
# cell's values are a function of the contig's window base, so that they sit
# at exact distances from the window's edges.
#
# The base depends on the reads, which depend on the values.  To make that
# circle close, a segment's reads are built so that the bases cannot see the
# values: the plateau's reads (reads_for_profile) end before the segment; F
# floor reads span the whole segment; every position p of it then gets
# v[p] - F reads of span 1; and the bump positions take as many span-1 reads
# as bring the segment's count to a fixed N (BAND per position for base - F,
# plus the values' offsets from the base, which no base changes).  With F
# fixed, every read's tid and span and its index in the batch are the same
# whatever the values are, and the window bases (which read no positions)
# with them.  build() moves F only when base - F leaves [BAND_MIN, BAND],
# iterates to the fixed point and fails if there is none.

RAMP = 16
TAIL = 8
BUMP = 16
BG_SPAN = 32                            # the plateau's reads
BAND, BAND_AIM, BAND_MIN = 120, 75, 35   # base - F stays in [BAND_MIN, BAND]: values reach down to base - 30
VARIANTS = ("full", "direct", "long")   # the three ways the GPU tests run a case set
LONG_CONTIG = 8192                      # the extra contig of the long variant
LONG_SPAN = 5000                        # and its one read: > K_SHORT_MAX


class Item:
    def __init__(self, fn, n, region=True, zx=0, tag=None, want=None):
        self.fn, self.n, self.region, self.zx, self.tag, self.want = fn, n, region, zx, tag, want


def cell(fn, n, **kw):
    return Item(fn, n, True, **kw)


def pad(n, off=400):
    """n positions that belong to no region (off: their value above the base)."""
    return Item(lambda b, d: np.full(n, max(0, b + off), np.int64), n, False)


def bump(n=BUMP):
    return Item(None, n, False)


class Contig:
    def __init__(self, depth, lead, segments, start_base=None, end_open=False, plain=False, zero=False,
                 floor_above=0, overhang=0):
        # lead: the positions before the first cell (ramp, plateau and the
        #   first segment's bump, unless the segment places its own)
        # end_open: the contig ends with its last item (no tail), whose region
        #   may run `zx` positions past the contig end
        # plain: items only, as span-1 reads (a tiny contig; its read count
        #   follows its values)
        # zero: the cells' values are absolute and the window base must come out as 0
        # floor_above: the floor follows base + floor_above (no value is below that)
        # overhang: the contig's length is this much shorter than its reads reach (its extent)
        self.floor_above, self.zero, self.overhang = floor_above, zero, overhang
        if segments and isinstance(segments[0], Item):
            segments = [segments]
        self.segments = []
        for k, s in enumerate(segments):
            s = list(s)
            if not plain and not any(i.fn is None for i in s):
                assert k == 0
                s = [bump()] + s
                lead -= BUMP
            assert plain or sum(1 for i in s if i.fn is None) == 1
            assert sum(i.n for i in s) <= K_SHORT_MAX      # the floor reads span the segment
            self.segments.append(s)
        self.depth, self.lead, self.start_base, self.end_open, self.plain = depth, lead, start_base, end_open, plain
        assert plain or lead >= RAMP
        self.zone = sum(i.n for s in self.segments for i in s)
        self._bg = None

    def length(self):
        return self.lead + self.zone + (0 if self.end_open or self.plain else TAIL + RAMP)

    def background(self):
        """The plateau's profile and reads (nothing in the segments)."""
        if self._bg is None:
            d = self.depth
            parts = [np.zeros(self.zone, np.int64)]
            if not self.plain:
                up = (np.arange(1, RAMP + 1, dtype=np.int64) * d) // RAMP
                parts = [up, np.full(self.lead - RAMP, d, np.int64)] + parts
                if not self.end_open:
                    parts += [np.full(TAIL, d, np.int64), ((np.arange(RAMP, 0, -1, dtype=np.int64) - 1) * d) // RAMP]
            prof = np.concatenate(parts)
            assert len(prof) == self.length()
            self._bg = (prof,) + reads_for_profile(prof, BG_SPAN)
        return self._bg

    def needed(self, base, floor):
        """Span-1 reads each segment's cells and pads take."""
        out = []
        for s in self.segments:
            k = 0
            for i in s:
                if i.fn is not None:
                    v = np.asarray(i.fn(int(base), self.depth), np.int64)
                    assert len(v) == i.n and v.min() >= floor, (i.tag, int(v.min()), floor)
                    k += int((v - floor).sum())
            out.append(k)
        return out

    def assemble(self, base, floor, counts):
        """(profile, pos, span) with `floor` floor reads and counts[k] span-1
        reads in segment k."""
        prof, bpos, bspan = self.background()
        prof = prof.copy()
        pos, span = [bpos.astype(np.int64)], [bspan.astype(np.int64)]
        at = self.lead
        for s, n_seg in zip(self.segments, counts):
            seg_len = sum(i.n for i in s)
            vals = np.zeros(seg_len, np.int64)
            k, used, bump_at = 0, 0, None
            for i in s:
                if i.fn is None:
                    bump_at = (k, i.n)
                else:
                    v = np.asarray(i.fn(int(base), self.depth), np.int64)
                    vals[k:k + i.n] = v - floor
                    used += int((v - floor).sum())
                k += i.n
            if bump_at is not None:
                left = n_seg - used
                assert left >= 0
                k, z = bump_at
                vals[k:k + z] = left // z + (np.arange(z) < left % z)
            else:
                assert n_seg == used
            pos += [np.full(floor, at, np.int64), np.repeat(at + np.arange(seg_len, dtype=np.int64), vals)]
            span += [np.full(floor, seg_len, np.int64), np.ones(int(vals.sum()), np.int64)]
            prof[at:at + seg_len] = floor + vals
            at += seg_len
        pos, span = np.concatenate(pos), np.concatenate(span)
        o = np.argsort(pos, kind="stable")     # at one position: plateau, floor, span-1 reads
        return prof, pos[o].astype(np.int32), span[o].astype(np.int32)


class Built:
    """A case set built for one variant: the batch, the regions, the model's
    bases and the depth the reads give."""


def _bases(variant, extent, tid, span, params=None):
    if variant == "direct":
        return window_base_direct(extent, tid, span, params)      # (direct batches have extent == length)
    return window_base_full(extent, tid, span, params)


def build(contigs, variant, extra_regions=(), long_read=None):
    """Reads for a case set.  variant: "full" (the full prepare's window
    bases), "direct" (the probe's) or "long" (full, with one long read on an
    extra contig; long_read adds that contig to another variant)."""
    assert variant in VARIANTS
    if long_read is None:
        long_read = variant == "long"
    base_variant = "full" if variant == "long" else variant
    nc = len(contigs)
    extent = np.array([c.length() for c in contigs] + ([LONG_CONTIG] if long_read else []), np.int64)
    lengths = extent - np.array([c.overhang for c in contigs] + ([0] if long_read else []), np.int64)
    assert base_variant == "full" or np.array_equal(lengths, extent)
    base = [int(c.start_base if c.start_base is not None else max(0, c.depth - K_WIN_BELOW)) for c in contigs]
    # the span-1 reads of every segment: BAND per position for base - floor,
    # plus the values' offsets from the base (which no base changes)
    far = 1 << 20
    counts = [c.needed(b, 0) if c.zero or c.plain else c.needed(far, far - BAND + c.floor_above)
              for c, b in zip(contigs, base)]
    floor = [0 if c.zero or c.plain else max(0, b + c.floor_above - BAND_AIM) for c, b in zip(contigs, base)]
    for _ in range(64):
        parts = [c.assemble(b, f, k) for c, b, f, k in zip(contigs, base, floor, counts)]
        profiles = [p[0] for p in parts]
        tids = [np.full(len(p[1]), t, np.int32) for t, p in enumerate(parts)]
        poss, spans = [p[1] for p in parts], [p[2] for p in parts]
        if long_read:
            profiles.append(np.concatenate([np.ones(LONG_SPAN, np.int64), np.zeros(LONG_CONTIG - LONG_SPAN, np.int64)]))
            tids.append(np.array([nc], np.int32))
            poss.append(np.array([0], np.int32))
            spans.append(np.array([LONG_SPAN], np.int32))
        tid, pos, span = np.concatenate(tids), np.concatenate(poss), np.concatenate(spans)
        new = [int(x) for x in _bases(base_variant, extent, tid, span)[:nc]]
        if new == base:
            break
        base = new
        for t, c in enumerate(contigs):
            if c.plain:
                counts[t] = c.needed(base[t], 0)
            elif c.zero:
                assert base[t] == 0, "contig %d: its window base should be 0" % t
            else:
                assert base[t] + c.floor_above >= BAND, "contig %d: window base %d too low" % (t, base[t])
                if not BAND_MIN <= base[t] + c.floor_above - floor[t] <= BAND:
                    floor[t] = base[t] + c.floor_above - BAND_AIM
    else:
        raise AssertionError("the window bases reached no fixed point")
    b = Built()
    b.variant, b.base_variant, b.contigs, b.long_read = variant, base_variant, contigs, long_read
    b.lengths, b.extent, b.tid, b.pos, b.span, b.profiles = lengths, extent, tid, pos, span, profiles
    b.base = _bases(base_variant, extent, tid, span)
    b.floor, b.counts = floor, counts
    rt, rs, re_, items = [], [], [], []
    for t, c in enumerate(contigs):
        at = c.lead
        for s in c.segments:
            for i in s:
                if i.region:
                    rt.append(t)
                    rs.append(at)
                    re_.append(at + i.n + i.zx)
                    items.append(i)
                at += i.n
    for t, s, e in extra_regions:
        rt.append(t)
        rs.append(s if s >= 0 else int(extent[t]) - s - 1)    # s < 0: -s - 1 past the contig's extent
        re_.append(rs[-1] + e)                                # e: the region's length
        items.append(None)
    b.rtid, b.rs, b.re, b.items = np.array(rt, np.int32), np.array(rs, np.int64), np.array(re_, np.int64), items
    return b


def model_rows(b, params=None, sel=None):
    """(bases, info) of the built case set's regions under `params`: info[r]
    is classify()'s result for region r (of `sel`, default all)."""
    base = _bases(b.base_variant, b.extent, b.tid, b.span, params)
    info = []
    for r in (range(len(b.rtid)) if sel is None else sel):
        t = int(b.rtid[r])
        ext = int(b.extent[t])
        a, e = min(int(b.rs[r]), ext), min(int(b.re[r]), ext)
        zx = int(b.re[r] - b.rs[r]) - (e - a)
        info.append(classify(b.profiles[t], a, e, int(base[t]), zx, params))
    return base, info


# ---- cells -----------------------------------------------------------------

W = K_HIST_BINS


def _spread(b, k):
    """k values inside the window, its first and last value among them."""
    if k <= 0:
        return np.zeros(0, np.int64)
    if k == 1:
        return np.array([b + W - 1], np.int64)
    return b + (np.arange(k, dtype=np.int64) * (W - 1)) // (k - 1)


def rank_cell(n, lo, hi, flip, zx=0, **kw):
    """n positions (zx of them past the extent): lo values just below the
    window (base - 1), hi just above (base + 864), the rest spread over it."""
    real = n - zx

    def fn(b, d):
        v = np.concatenate([np.full(lo, b - 1, np.int64), _spread(b, real - lo - hi), np.full(hi, b + W, np.int64)])
        return v[::-1] if flip else v
    return cell(fn, real, zx=zx, **kw)


def rank_edge_cells(base_zero=False):
    """Cells with q_lo - win_lo in (-1, 0, +1) and (q_hi - 1) - win_hi in
    (-2, -1, 0), for n = 12 .. 15 and 1 .. 5, wherever the counts fit.  On a
    contig of base 0 nothing can lie below the window: only the high side."""
    out = []
    for n in (12, 13, 14, 15, 1, 2, 3, 4, 5):
        for dl in ((None,) if base_zero else (-1, 0, 1)):
            for dh in (-2, -1, 0):
                lo = 0 if dl is None else n // 4 - dl
                hi = n // 4 + 1 + dh
                if lo < 0 or hi < 0 or lo + hi > n:
                    continue
                out.append(rank_cell(n, lo, hi, len(out) % 2 == 1, tag="rank n=%d dl=%s dh=%d" % (n, dl, dh),
                                     want={"dl": dl, "dh": dh}))
    return out


def zx_rank_contig(depth, n, dl, dh=None):
    """A contig whose last region runs past its end: the ranks below the
    window are zeros past the extent only (q_lo - win_lo = dl)."""
    zx = n // 4 - dl
    hi = 0 if dh is None else n // 4 + 1 + dh
    c = rank_cell(n, 0, hi, False, zx=zx, tag="zx-rank n=%d dl=%d dh=%s" % (n, dl, dh), want={"dl": dl, "dh": dh})
    return Contig(depth, 256, [c], end_open=True)


def rank_edges_set(depth=3000, depth0=100):
    contigs = [Contig(depth, 512, rank_edge_cells()),
               Contig(depth0, 6000, rank_edge_cells(base_zero=True), zero=True)]
    for n, dl in ((13, -1), (14, 0), (13, 1)):
        contigs.append(zx_rank_contig(depth, n, dl))
    contigs.append(zx_rank_contig(depth, 15, 0, 0))
    contigs.append(zx_rank_contig(depth, 12, 1, -1))
    return contigs, ()


def _runs(x, y, r, n):
    """x, y alternating in runs of r, n values."""
    k = np.arange(n) // r
    return np.where(k % 2 == 0, x, y).astype(np.int64)


def value_edges_set(depth=3000, depth0=100):
    """Values alternating across the window's edges in runs of 1 .. 4, at every
    alignment modulo 4, in cells whose lengths are no multiple of 4: dense
    cells (13 positions, half of them outside: mostly flagged) and sparse
    ones (the runs among values inside the window: not flagged)."""
    items = []
    lead = 512
    at = lead
    for pair in ("high", "low"):
        for r in (1, 2, 3, 4):
            for a in (0, 1, 2, 3):
                for dense in (True, False):
                    if at % 4 != a:
                        k = (a - at) % 4
                        items.append(pad(k))
                        at += k
                    n = 13 if dense else 8 * r + 1
                    swap = (a + r) % 2 == 1

                    def fn(b, d, pair=pair, r=r, n=n, dense=dense, swap=swap):
                        x, y = (b + W - 1, b + W) if pair == "high" else (b, b - 1)
                        if swap:
                            x, y = y, x
                        if dense:
                            return _runs(x, y, r, n)
                        v = b + 300 + (np.arange(n, dtype=np.int64) * 37) % 200
                        # 2 r positions outside the window: q_lo = n / 4 = 2 r holds them
                        k0 = (n - 4 * r) // 2
                        v[k0:k0 + 4 * r] = _runs(x, y, r, 4 * r)
                        return v
                    items.append(cell(fn, n, tag="%s r=%d a=%d %s" % (pair, r, a, "dense" if dense else "sparse")))
                    at += n
    items.append(pad((-at) % 4 + 1))
    items.append(cell(lambda b, d: b + W + np.arange(7, dtype=np.int64) % 3, 7, tag="all above"))
    items.append(cell(lambda b, d: b - 1 - np.arange(7, dtype=np.int64) % 3, 7, tag="all below"))
    items.append(cell(lambda b, d: np.array([b - 1, b + W, b - 2, b + W + 5, b + W, b - 1], np.int64), 6,
                      tag="below and above, none inside"))
    items.append(cell(lambda b, d: np.array([b, b - 1, b + W - 1, b + W, b, b - 1, b + W - 1, b + W, b + 5], np.int64),
                      9, tag="all four edge values"))
    # base 0: nothing below; 863 / 864 alternate
    items0 = []
    for r in (1, 2, 3, 4):
        items0.append(cell(lambda b, d, r=r: _runs(W - 1, W, r, 13), 13, tag="base0 dense r=%d" % r))
        items0.append(pad(r))

        def fn0(b, d, r=r):
            n = 8 * r + 1
            v = 100 + (np.arange(n, dtype=np.int64) * 37) % 200
            k0 = (n - 4 * r) // 2
            v[k0:k0 + 4 * r] = _runs(W, W - 1, r, 4 * r)
            return v
        items0.append(cell(fn0, 8 * r + 1, tag="base0 sparse r=%d" % r))
    items0.append(cell(lambda b, d: np.full(5, W, np.int64), 5, tag="base0 all above"))
    return [Contig(depth, lead, items), Contig(depth0, 6000, items0, zero=True)], ()


def compose_set(depth=3000, depth0=100, full_only=True):
    """Minimum / maximum composition, zeros past the extent, empty regions,
    a tiny contig whose depth estimate is an exact half, and a contig whose
    reads run past its length."""
    def inwin(n):
        return lambda b, d: b + 100 + (np.arange(n, dtype=np.int64) * 131) % 600

    def with_(n, lows, highs):
        def fn(b, d):
            v = b + 100 + (np.arange(n, dtype=np.int64) * 131) % 600
            v[1:1 + len(lows)] = b - np.array(lows, np.int64)
            v[n - 1 - len(highs):n - 1] = b + W - 1 + np.array(highs, np.int64)
            return v
        return fn
    main = [cell(with_(9, [1, 7], []), 9, tag="low real, unflagged"),
            cell(with_(9, [], [1, 30]), 9, tag="high only, unflagged"),
            cell(with_(13, [3, 1], [2, 1]), 13, tag="low and high, unflagged"),
            cell(inwin(11), 11, tag="inside only"),
            cell(lambda b, d: b + np.array([0, W - 1, 3, W - 1, 0], np.int64), 5, tag="edge values inside"),
            cell(with_(9, [1, 2, 3], []), 9, tag="low real, flagged"),
            pad(3),
            cell(with_(10, [], [1, 2, 3]), 10, tag="high, flagged")]
    zx_c = Contig(depth, 256, [cell(inwin(9), 9, zx=3, tag="zx only below, unflagged")], end_open=True)
    zx_h = Contig(depth, 256, [cell(with_(9, [], [4, 9]), 9, zx=3, tag="zx below, high above")], end_open=True)
    zx_l = Contig(depth, 256, [cell(with_(12, [5], []), 12, zx=2, tag="zx and real below")], end_open=True)
    zx_f = Contig(depth, 256, [cell(inwin(6), 6, zx=9, tag="zx below, flagged")], end_open=True)
    zero = Contig(depth0, 3000, [cell(lambda b, d: np.array([5, W - 1, W, 40, 7, 9, 2000, 3, 11], np.int64), 9,
                                     tag="base0 high"),
                                cell(lambda b, d: np.array([0, 5, 0, 9, W - 1], np.int64), 5, tag="base0 real zeros")], zero=True)
    zero_zx = Contig(depth0, 3000, [cell(lambda b, d: np.array([17, 30, W - 1, 4, 8, 100], np.int64), 6, zx=5,
                                        tag="base0 zx in bin 0")], end_open=True, zero=True)
    zero_zxh = Contig(depth0, 3000, [cell(lambda b, d: np.array([17, W, W + 9, 4, 8, 100, 3, 2], np.int64), 8, zx=4,
                                         tag="base0 zx and high")], end_open=True, zero=True)
    # est = base + 648.5 whatever the base (the extent is below two mean
    # spans: body = extent): llrint keeps the even start base, llround would
    # raise it by one, which moves the value `base` of the first region out
    tie = Contig(0, 0, [cell(lambda b, d: np.array([b], np.int64), 1, tag="tie base"),
                        cell(lambda b, d: b + np.array([741, 741, 741, 742, 741, 741, 741], np.int64), 7,
                             tag="tie rest")], start_base=2000, plain=True)
    # reads run 4 positions past the contig's length: the extent, not the
    # length, gives the base; single values on both of the window's edges
    over = Contig(depth, 256, [cell(lambda b, d: np.array([b], np.int64), 1, tag="overhang base"),
                               cell(lambda b, d: np.array([b + W - 1], np.int64), 1, tag="overhang base+863"),
                               cell(inwin(9), 9, zx=3, tag="overhang zx")], end_open=True, overhang=4)
    contigs = [Contig(depth, 512, main), zx_c, zx_h, zx_l, zx_f, zero, zero_zx, zero_zxh] + ([tie, over] if full_only else [])
    extra = [(0, -1, 5), (0, -41, 1), (5, -3, 7), (0, 7, 0), (5, 4000, 0), (1, -1, 0)]
    return contigs, extra


def tiny_set(depth=3000):
    """4096 one-position regions that cover exactly one tile, their values a
    triangle wave over [base - 3, base + 866], then regions of 1 .. 3
    positions that share int4s, a third of their values outside the window."""
    def tri(b, d):
        k = np.arange(K_TILE_W, dtype=np.int64) % (2 * 869)
        return b - 3 + np.minimum(k, 2 * 869 - k)
    wave = []
    for i in range(K_TILE_W):
        wave.append(cell(lambda b, d, i=i: tri(b, d)[i:i + 1], 1))
    edge = (-1, 0, W - 1, W, 200, 431, W + 2, 77, -2, 650, 300, 12)
    small, at = [], 0
    for k in range(90):
        n = (1, 3, 2, 2, 3, 1, 1)[k % 7]
        small.append(cell(lambda b, d, at=at, n=n: b + np.array([edge[(at + q) * 5 % 12] for q in range(n)], np.int64),
                          n, tag="small %d" % k))
        at += n
        if k % 11 == 10:
            small.append(pad(1))
            at += 1
    half = K_TILE_W // 2
    return [Contig(depth, K_TILE_W - 64, [[bump(64)] + wave[:half], wave[half:] + small + [bump(64)]])], ()


def chunk_set(depth=2500):
    """Regions across a tile boundary (4096) and across chunk boundaries
    (8192 and 16384 in the global layout), values outside the window on both
    sides of each boundary; the last one is flagged."""
    def mix(n, cut, lows, highs):
        # lows / highs: offsets from the boundary at `cut`
        def fn(b, d):
            v = b + 50 + (np.arange(n, dtype=np.int64) * 53) % 700
            v[0], v[n - 1] = b, b + W - 1
            for o in lows:
                v[cut + o] = b - 1 - (o % 3)
            for o in highs:
                v[cut + o] = b + W + (o % 5)
            return v
        return fn
    c0 = Contig(depth, 4096 - 30, [
        [cell(mix(71, 30, [-3, -1, 2], [-2, 0, 1]), 71, tag="across the tile boundary"), pad(2000, -30)],
        [pad(8192 - 37 - (4096 - 30 + 71) - 2000, -30),
         cell(mix(78, 37, [-4, -1, 0, 3], [-2, 1, 2, 9]), 78, tag="across chunk boundary 8192"), bump()]])
    len0 = c0.length()
    assert len0 == 8192 + 41 + BUMP + TAIL + RAMP
    off1 = (len0 + 63) // 64 * 64
    lead1 = 16384 - off1 - 21
    c1 = Contig(depth, lead1, [
        cell(mix(50, 21, [-9, -8, -7, -6, -5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5], [-12, -11, 8, 9]), 50,
             tag="across chunk boundary 16384, flagged")])
    return [c0, c1], ()


def slot_set(depth=3000, n_flag=K_FB_SLOTS + 1, n_plain=24):
    """n_flag flagged 8-position cells (four values above the window) and
    n_plain unflagged ones after them."""
    items = []
    for k in range(n_flag):
        items.append(cell(lambda b, d, k=k: b + W - 4 + (np.arange(8, dtype=np.int64) + k) % 8, 8, tag="slot flagged"))
    for k in range(n_plain):
        items.append(cell(lambda b, d, k=k: b + W - 9 + (np.arange(8, dtype=np.int64) + k) % 8 + (np.arange(8) == k % 8),
                          8, tag="slot plain"))
    return [Contig(depth, 512, [items[:256], items[256:] + [bump()]], floor_above=840),
            Contig(100, 3000, [cell(lambda b, d: np.arange(8, dtype=np.int64) * 100, 8)], zero=True)], ()


CASE_SETS = {
    "rank_edges": rank_edges_set,
    "value_edges": value_edges_set,
    "compose": compose_set,
    "tiny": tiny_set,
    "chunk": chunk_set,
    "slot": slot_set,
}

_BUILT = {}


def built(name, variant, long_read=None, **kw):
    """The case set `name` built for `variant`, once per process."""
    if name == "compose" and variant == "direct":
        kw["full_only"] = False    # (no exact half in the probe's estimate; no read past a contig's end)
    key = (name, variant, long_read, tuple(sorted(kw.items())))
    if key not in _BUILT:
        contigs, extra = CASE_SETS[name](**kw)
        _BUILT[key] = build(contigs, variant, extra, long_read)
    return _BUILT[key]
