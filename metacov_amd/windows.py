"""Windowed coverage: per-window depth sums and threshold counts, and the
depth histogram per segment.

    wc = eng.depth_windows(window=500, thresholds="1,10,30")   # every contig over [0, length)
    wc = eng.depth_windows(tids, starts, ends)                 # window=0: one row per segment
    write_windows_bed(wc, names, fh)
    hist = eng.depth_hist(n_bins=1024)                         # int64 [S, n_bins]
    write_dist(hist, names, fh)

The form between the nine statistics per region (`pileup`) and the per-base
runs (`depth`): mean depth in fixed windows (mosdepth --by, deepTools bins),
breadth of coverage (mosdepth --thresholds, CoverM's covered fraction) and the
cumulative depth distribution (mosdepth's *.dist.txt).  Everything is one
streaming read of the depth vector `compute_depth` left in HBM
(csrc/windows.hip, mc_windows_* in include/metacov_amd.h); only the rows cross
to the host.  Integer arithmetic throughout: results are exact.  The reference
has no counterpart.  Depths are exact int32 values: the pileup read cap of
`metacov pileup` is not applied here.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check, ptr

MAX_THRESHOLDS = 16
MIN_WINDOW = 16


def parse_thresholds(spec):
    """"1,10,30" -> [1, 10, 30]: at most 16 non-negative, strictly increasing
    int32 depths separated by ','.  An empty spec is no threshold."""
    if not isinstance(spec, str):
        raise ValueError("thresholds spec must be a string like '1,10,30'")
    if spec.strip() == "":
        return []
    parts = [p.strip() for p in spec.split(",")]
    if any(not p.isdigit() for p in parts):
        raise ValueError("thresholds spec %r: depths must be non-negative integers separated by ','" % spec)
    thr = [int(p, 10) for p in parts]
    if any(b <= a for a, b in zip(thr, thr[1:])):
        raise ValueError("thresholds spec %r: depths must be strictly increasing" % spec)
    if len(thr) > MAX_THRESHOLDS:
        raise ValueError("thresholds spec %r: more than %d depths" % (spec, MAX_THRESHOLDS))
    if thr[-1] > np.iinfo(np.int32).max:
        raise ValueError("thresholds spec %r: depths must fit int32" % spec)
    return thr


def _thresholds(thresholds):
    """int32 array of a thresholds argument (None, a spec string or a sequence)."""
    if thresholds is None:
        return np.zeros(0, np.int32)
    if isinstance(thresholds, str):
        thresholds = parse_thresholds(thresholds)
    t = np.asarray(thresholds)
    if t.ndim != 1 or (t.size and not np.issubdtype(t.dtype, np.integer)):
        raise ValueError("thresholds must be a 1-d integer sequence")
    if t.size and (t.min() < np.iinfo(np.int32).min or t.max() > np.iinfo(np.int32).max):
        raise ValueError("thresholds must fit int32")
    return np.ascontiguousarray(t, dtype=np.int32)


class WindowCoverage:
    """Windows of S segments, in segment order.

    tids / starts / seg_ends: the segments (int32 / int64 / int64).
    window: the window length (0: one window per non-empty segment).
    thresholds [n_thr] int32.
    seg_first [S + 1]: segment i owns windows seg_first[i] .. seg_first[i + 1].
    sum [n] int64: each window's sum of depths.
    ge [n, n_thr] int64: its positions with depth >= thresholds[j]."""

    def __init__(self, tids, starts, ends, window, thresholds, seg_first, sum, ge):
        self.tids = np.asarray(tids, np.int32)
        self.starts = np.asarray(starts, np.int64)
        self.seg_ends = np.asarray(ends, np.int64)
        self.window = int(window)
        self.thresholds = np.asarray(thresholds, np.int32)
        self.seg_first = np.asarray(seg_first, np.int64)
        self.sum = np.asarray(sum, np.int64)
        self.ge = np.asarray(ge, np.int64).reshape(len(self.sum), len(self.thresholds))
        if len(self.seg_first) != len(self.tids) + 1 or (len(self.seg_first) and self.seg_first[-1] != len(self.sum)):
            raise ValueError("inconsistent WindowCoverage arrays")

    def __len__(self):
        return len(self.sum)

    @property
    def n_segments(self):
        return len(self.tids)

    def segment_of(self):
        """int64 [n]: each window's segment."""
        return np.repeat(np.arange(len(self.tids), dtype=np.int64), np.diff(self.seg_first))

    def start(self):
        """int64 [n]: each window's first position, relative to its contig."""
        seg = self.segment_of()
        k = np.arange(len(self.sum), dtype=np.int64) - self.seg_first[:-1][seg]
        return self.starts[seg] + k * self.window

    def end(self):
        """int64 [n]: each window's end (exclusive)."""
        seg = self.segment_of()
        if self.window == 0:
            return self.seg_ends[seg]
        return np.minimum(self.start() + self.window, self.seg_ends[seg])

    def length(self):
        return self.end() - self.start()

    def mean(self):
        """float64 [n]: sum / length."""
        return self.sum / self.length()


class WindowsHandle:
    """One mc_windows (device buffers that only grow, reused between calls)."""

    def __init__(self, device=0, lib=None):
        self._lib = lib or _lib.load()
        self._h = ctypes.c_void_p()
        check(self._lib.mc_windows_create(int(device), ctypes.byref(self._h)), self._lib)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mc_windows_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def compute(self, ctx, tids, starts, ends, window, thr):
        """-> (n_windows, seg_first); the rows stay on the device (get())."""
        n = ctypes.c_int64()
        check(self._lib.mc_windows_compute(self._h, ctx, len(tids), ptr(tids), ptr(starts), ptr(ends),
                                           int(window), len(thr), ptr(thr), ctypes.byref(n)), self._lib)
        seg_first = np.zeros(len(tids) + 1, np.int64)
        check(self._lib.mc_windows_seg_first(self._h, ptr(seg_first)), self._lib)
        self._n_thr = len(thr)
        return n.value, seg_first

    def get(self, first, count):
        s = np.empty(count, np.int64)
        ge = np.empty((count, self._n_thr), np.int64)
        check(self._lib.mc_windows_get(self._h, int(first), int(count), ptr(s),
                                       ptr(ge) if self._n_thr else None), self._lib)
        return s, ge

    def hist(self, ctx, tids, starts, ends, n_bins):
        out = np.zeros((len(tids), int(n_bins)), np.int64)
        check(self._lib.mc_windows_hist(self._h, ctx, len(tids), ptr(tids), ptr(starts), ptr(ends),
                                        int(n_bins), ptr(out)), self._lib)
        return out

    def timing(self):
        a, b, c = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        t = ctypes.c_int64()
        check(self._lib.mc_windows_timing(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                                          ctypes.byref(t)), self._lib)
        return {"window_ms": a.value, "combine_ms": b.value, "hist_ms": c.value, "tiles": t.value}


def dims(lib=None):
    """(tile positions, smallest window, most bins, histogram workgroups) of the kernels."""
    lib = lib or _lib.load()
    v = [ctypes.c_int32() for _ in range(4)]
    check(lib.mc_windows_dims(*(ctypes.byref(x) for x in v)), lib)
    return tuple(x.value for x in v)


def _segments(eng, tids, starts, ends):
    """depth_runs' defaults: every contig over [0, length)."""
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
    return tids, starts, ends


def _handle(eng):
    if eng._windows is None:
        eng._windows = WindowsHandle(eng.device, eng._lib)
    return eng._windows


def depth_windows(eng, tids=None, starts=None, ends=None, window=0, thresholds=None):
    """CoverageEngine.depth_windows (see there)."""
    tids, starts, ends = _segments(eng, tids, starts, ends)
    thr = _thresholds(thresholds)
    h = _handle(eng)
    n, seg_first = h.compute(eng._h, tids, starts, ends, window, thr)
    s, ge = h.get(0, n)
    return WindowCoverage(tids, starts, ends, window, thr, seg_first, s, ge)


def depth_hist(eng, tids=None, starts=None, ends=None, n_bins=1024):
    """CoverageEngine.depth_hist (see there)."""
    tids, starts, ends = _segments(eng, tids, starts, ends)
    return _handle(eng).hist(eng._h, tids, starts, ends, n_bins)


def write_windows_bed(wc, names, fh, header=True):
    """Tab-separated `name start end mean` lines, one window per line, in
    order; the mean as '%.2f' % (sum / length).  With thresholds a header line
    `#chrom start end mean 1X 10X ...` comes first (header=False: not, for
    the later parts of one file) and one integer column per threshold (the
    positions at or above it) is appended.  names[tid]: the contig names.
    Returns the windows written."""
    thr = wc.thresholds.tolist()
    if thr and header:
        fh.write("\t".join(["#chrom", "start", "end", "mean"] + ["%dX" % t for t in thr]) + "\n")
    n = len(wc)
    if n == 0:
        return 0
    seg = wc.segment_of()
    start, end = wc.start(), wc.end()
    name = np.array([str(names[int(t)]) for t in wc.tids], dtype=object)[seg]
    total, length, ge = wc.sum.tolist(), (end - start).tolist(), wc.ge.tolist()
    start, end = start.tolist(), end.tolist()
    lines = []
    for i in range(n):
        cols = [name[i], str(start[i]), str(end[i]), "%.2f" % (total[i] / length[i])]
        cols += [str(c) for c in ge[i]]
        lines.append("\t".join(cols))
    fh.write("\n".join(lines))
    fh.write("\n")
    return n


def write_dist(hist, labels, fh):
    """The cumulative depth distribution of every row of hist [S, n_bins], then
    of their column sum under the label `total`: lines `label depth fraction`
    from the highest non-empty bin down to 0, fraction = positions with depth
    >= depth over all positions, as '%.4f'.  The last bin holds every depth at
    or above n_bins - 1 and is written as `N+`.  A row of length 0 writes
    nothing.  Returns the lines written."""
    hist = np.asarray(hist, np.int64)
    if hist.ndim != 2 or len(hist) != len(labels):
        raise ValueError("hist must be [len(labels), n_bins]")
    n_bins = hist.shape[1]
    written = 0
    rows = [(str(lab), hist[i]) for i, lab in enumerate(labels)]
    rows.append(("total", hist.sum(axis=0)))
    for lab, row in rows:
        n = int(row.sum())
        if n == 0:
            continue
        top = int(np.flatnonzero(row)[-1])
        cum = np.cumsum(row[::-1])[::-1].tolist()       # cum[b]: positions with depth >= b
        lines = []
        for b in range(top, -1, -1):
            depth = "%d+" % b if b == n_bins - 1 else "%d" % b
            lines.append("%s\t%s\t%.4f" % (lab, depth, cum[b] / n))
        fh.write("\n".join(lines))
        fh.write("\n")
        written += len(lines)
    return written
