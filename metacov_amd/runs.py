"""Per-base depth as runs: the bedGraph form of the depth vector.

    runs = eng.depth_runs()                        # every contig over [0, length)
    runs = eng.depth_runs(tids, starts, ends, quantize="0:1:4:100:")
    write_bedgraph(runs, names, fh, zero=False)

The run-length compaction runs on the GPU (csrc/runs.hip, mc_runs_* in
include/metacov_amd.h) over the depth vector `compute_depth` left in HBM;
only the runs (12 bytes each) cross to the host.  This is the output
`bedtools genomecov -bg/-bga`, `mosdepth` and `samtools depth` write; the
reference has no counterpart (its pileup reports region statistics only).
Depths are exact int32 values: the pileup read cap of `metacov pileup`
(metacov_amd.depthcap) is a per-query artefact and is not applied here.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check, ptr

MAX_EDGES = 16


def parse_quantize(spec):
    """mosdepth's --quantize grammar: "0:1:4:100:" -> (edges, labels) =
    ([1, 4, 100], ["0:1", "1:4", "4:100", "100:inf"]).

    Bounds are strictly increasing integers separated by ':'.  The first must
    be 0 (a depth below the first bound would have no class) and at least one
    more must follow; at most 16 follow it.  class(d) = number of edges <= d.
    A trailing ':' opens the last class ("100:inf").  Without it the depths
    at or above the last bound belong to no class: their label is None, and
    write_bedgraph leaves such runs out (as mosdepth does)."""
    if not isinstance(spec, str):
        raise ValueError("quantize spec must be a string like '0:1:4:100:'")
    parts = spec.strip().split(":")
    open_last = len(parts) > 1 and parts[-1] == ""
    if open_last:
        parts = parts[:-1]
    try:
        bounds = [int(p, 10) for p in parts]
    except ValueError:
        raise ValueError("quantize spec %r: bounds must be integers separated by ':'" % spec) from None
    if any(not p.strip().isdigit() for p in parts):
        raise ValueError("quantize spec %r: bounds must be non-negative integers" % spec)
    if bounds[0] != 0:
        raise ValueError("quantize spec %r: the first bound must be 0" % spec)
    if len(bounds) < 2:
        raise ValueError("quantize spec %r: needs at least one bound after 0" % spec)
    if any(b <= a for a, b in zip(bounds, bounds[1:])):
        raise ValueError("quantize spec %r: bounds must be strictly increasing" % spec)
    edges = bounds[1:]
    if len(edges) > MAX_EDGES:
        raise ValueError("quantize spec %r: more than %d bounds after 0" % (spec, MAX_EDGES))
    if edges[-1] > np.iinfo(np.int32).max:
        raise ValueError("quantize spec %r: bounds must fit int32" % spec)
    labels = ["%d:%d" % (a, b) for a, b in zip(bounds, bounds[1:])]
    labels.append("%d:inf" % bounds[-1] if open_last else None)
    return edges, labels


def _edges(quantize):
    """int32 edge array of a quantize argument (None, a spec string or a
    sequence of edges)."""
    if quantize is None:
        return np.zeros(0, np.int32)
    if isinstance(quantize, str):
        quantize = parse_quantize(quantize)[0]
    e = np.asarray(quantize)
    if e.ndim != 1 or (e.size and not np.issubdtype(e.dtype, np.integer)):
        raise ValueError("quantize edges must be a 1-d integer sequence")
    if e.size and (e.min() < np.iinfo(np.int32).min or e.max() > np.iinfo(np.int32).max):
        raise ValueError("quantize edges must fit int32")
    return np.ascontiguousarray(e, dtype=np.int32)


class DepthRuns:
    """Runs of equal (quantised) depth of S segments, in segment order.

    tids / starts / ends: the segments (int32 / int64 / int64).
    seg_first [S + 1]: segment i owns runs seg_first[i] .. seg_first[i + 1].
    start [n] int64: each run's first position, relative to its contig.
    value [n] int32: its depth (or class, when quantised).
    A run ends where the next run of its segment starts, or at the segment's
    end (ends()).  Zero runs are kept."""

    def __init__(self, tids, starts, ends, seg_first, start, value, edges=None):
        self.tids = np.asarray(tids, np.int32)
        self.starts = np.asarray(starts, np.int64)
        self.seg_ends = np.asarray(ends, np.int64)
        self.seg_first = np.asarray(seg_first, np.int64)
        self.start = np.asarray(start, np.int64)
        self.value = np.asarray(value, np.int32)
        self.edges = np.zeros(0, np.int32) if edges is None else np.asarray(edges, np.int32)
        if len(self.seg_first) != len(self.tids) + 1 or len(self.start) != len(self.value):
            raise ValueError("inconsistent DepthRuns arrays")

    def __len__(self):
        return len(self.start)

    @property
    def n_segments(self):
        return len(self.tids)

    def ends(self):
        """int64 [n]: each run's end (exclusive)."""
        e = np.empty(len(self.start), np.int64)
        e[:-1] = self.start[1:]
        full = self.seg_first[1:] > self.seg_first[:-1]
        e[self.seg_first[1:][full] - 1] = self.seg_ends[full]
        return e

    def segment(self, i):
        """(start, end, value) views of segment i's runs."""
        a, b = int(self.seg_first[i]), int(self.seg_first[i + 1])
        s = self.start[a:b]
        e = np.empty(b - a, np.int64)
        if b > a:
            e[:-1] = s[1:]
            e[-1] = self.seg_ends[i]
        return s, e, self.value[a:b]


class RunsHandle:
    """One mc_runs (device buffers that only grow, reused between calls)."""

    def __init__(self, device=0, lib=None):
        self._lib = lib or _lib.load()
        self._h = ctypes.c_void_p()
        check(self._lib.mc_runs_create(int(device), ctypes.byref(self._h)), self._lib)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mc_runs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def compute(self, ctx, tids, starts, ends, edges):
        """-> (n_runs, seg_first); the runs stay on the device (get())."""
        n = ctypes.c_int64()
        check(self._lib.mc_runs_compute(self._h, ctx, len(tids), ptr(tids), ptr(starts), ptr(ends),
                                        len(edges), ptr(edges), ctypes.byref(n)), self._lib)
        seg_first = np.zeros(len(tids) + 1, np.int64)
        check(self._lib.mc_runs_seg_first(self._h, ptr(seg_first)), self._lib)
        return n.value, seg_first

    def get(self, first, count):
        start = np.empty(count, np.int64)
        value = np.empty(count, np.int32)
        check(self._lib.mc_runs_get(self._h, int(first), int(count), ptr(start), ptr(value)), self._lib)
        return start, value

    def timing(self):
        c, s, e = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        t = ctypes.c_int64()
        check(self._lib.mc_runs_timing(self._h, ctypes.byref(c), ctypes.byref(s), ctypes.byref(e),
                                       ctypes.byref(t)), self._lib)
        return {"count_ms": c.value, "scan_ms": s.value, "emit_ms": e.value, "tiles": t.value}


def dims(lib=None):
    """(tile positions, tiles per scan iteration) of the kernels."""
    lib = lib or _lib.load()
    t, w = ctypes.c_int32(), ctypes.c_int32()
    check(lib.mc_runs_dims(ctypes.byref(t), ctypes.byref(w)), lib)
    return t.value, w.value


def depth_runs(eng, tids=None, starts=None, ends=None, quantize=None):
    """CoverageEngine.depth_runs (see there)."""
    if tids is None:
        if starts is not None or ends is not None:
            raise ValueError("starts / ends need tids")
        tids = np.arange(len(eng.lengths), dtype=np.int32)
        starts = np.zeros(len(tids), np.int64)
        ends = np.asarray(eng.lengths, np.int64)
    else:
        tids = np.ascontiguousarray(tids, dtype=np.int32)
        starts = (np.zeros(len(tids), np.int64) if starts is None
                  else np.ascontiguousarray(starts, dtype=np.int64))
        ends = (np.asarray(eng.lengths, np.int64)[tids] if ends is None
                else np.ascontiguousarray(ends, dtype=np.int64))
    tids, starts, ends = (np.ascontiguousarray(a) for a in (tids, starts, ends))
    if not len(tids) == len(starts) == len(ends):
        raise ValueError("tids / starts / ends lengths differ")
    edges = _edges(quantize)
    if eng._runs is None:
        eng._runs = RunsHandle(eng.device, eng._lib)
    n, seg_first = eng._runs.compute(eng._h, tids, starts, ends, edges)
    start, value = eng._runs.get(0, n)
    return DepthRuns(tids, starts, ends, seg_first, start, value, edges)


def write_bedgraph(runs, names, fh, zero=True, labels=None):
    """Tab-separated `name start end value` lines, one run per line, segment
    by segment in order.  names[tid]: the contig names.  zero=False leaves
    out the runs whose value is 0 (unquantised: depth 0; quantised: class 0).
    labels: the value column is labels[value] (parse_quantize's); runs whose
    label is None are left out.  Returns the lines written."""
    written = 0
    lab = None if labels is None else np.array(["" if x is None else x for x in labels], dtype=str)
    drop = None if labels is None else np.array([x is None for x in labels], bool)
    for i in range(runs.n_segments):
        s, e, v = runs.segment(i)
        if len(s) == 0:
            continue
        keep = None
        if not zero:
            keep = v != 0
        if drop is not None and drop.any():
            k2 = ~drop[v]
            keep = k2 if keep is None else keep & k2
        if keep is not None:
            s, e, v = s[keep], e[keep], v[keep]
            if len(s) == 0:
                continue
        col = lab[v] if lab is not None else v.astype(str)
        line = np.char.add(str(names[int(runs.tids[i])]) + "\t", s.astype(str))
        for c in (e.astype(str), col):
            line = np.char.add(np.char.add(line, "\t"), c)
        fh.write("\n".join(line.tolist()))
        fh.write("\n")
        written += len(s)
    return written
