"""Model of mc_windows_compute and mc_windows_hist (include/metacov_amd.h,
"windowed coverage") for the tests: numpy restatements, and a deliberately
naive per-position loop of each to check the restatements against.

All take the concatenated depth vector with each contig's extent and offset
(what oracle.coracle.depth returns) and the segments.  windows_* return
(seg_first, sum, ge) as the library does; hist_* return int64 [S, n_bins]."""
import numpy as np

from tests.runs_model import segment_vector


def windows_model(depth, ext, coff, tids, starts, ends, window, thr):
    thr = np.asarray([] if thr is None else thr, np.int64)
    seg_first = np.zeros(len(tids) + 1, np.int64)
    sums, ges = [], []
    for i, (t, a, b) in enumerate(zip(tids, starts, ends)):
        v = segment_vector(depth, ext, coff, int(t), int(a), int(b))
        n = len(v)
        if n == 0:
            seg_first[i + 1] = seg_first[i]
            continue
        w = n if window == 0 else int(window)
        at = np.arange(0, n, w)
        sums.append(np.add.reduceat(v, at))
        ges.append(np.stack([np.add.reduceat((v >= x).astype(np.int64), at) for x in thr], axis=1)
                   if len(thr) else np.zeros((len(at), 0), np.int64))
        seg_first[i + 1] = seg_first[i] + len(at)
    s = np.concatenate(sums).astype(np.int64) if sums else np.zeros(0, np.int64)
    ge = np.concatenate(ges).astype(np.int64) if ges else np.zeros((0, len(thr)), np.int64)
    return seg_first, s, ge


def windows_loop(depth, ext, coff, tids, starts, ends, window, thr):
    """The same, one position at a time."""
    thr = [] if thr is None else [int(x) for x in thr]
    seg_first, sums, ges = [0], [], []
    for t, a, b in zip(tids, starts, ends):
        t, a, b = int(t), int(a), int(b)
        for p in range(a, b):
            first = p == a if window == 0 else (p - a) % window == 0
            if first:
                sums.append(0)
                ges.append([0] * len(thr))
            d = int(depth[coff[t] + p]) if p < ext[t] else 0
            sums[-1] += d
            for j, x in enumerate(thr):
                if d >= x:
                    ges[-1][j] += 1
        seg_first.append(len(sums))
    return (np.array(seg_first, np.int64), np.array(sums, np.int64),
            np.array(ges, np.int64).reshape(len(sums), len(thr)))


def hist_model(depth, ext, coff, tids, starts, ends, n_bins):
    out = np.zeros((len(tids), n_bins), np.int64)
    for i, (t, a, b) in enumerate(zip(tids, starts, ends)):
        v = segment_vector(depth, ext, coff, int(t), int(a), int(b))
        out[i] = np.bincount(np.minimum(v, n_bins - 1), minlength=n_bins)
    return out


def hist_loop(depth, ext, coff, tids, starts, ends, n_bins):
    """The same, one position at a time."""
    out = np.zeros((len(tids), n_bins), np.int64)
    for i, (t, a, b) in enumerate(zip(tids, starts, ends)):
        t = int(t)
        for p in range(int(a), int(b)):
            d = int(depth[coff[t] + p]) if p < ext[t] else 0
            out[i, n_bins - 1 if d >= n_bins - 1 else d] += 1
    return out


def window_bounds(starts, ends, window):
    """(segment, start, end) of every window, in order."""
    seg, s, e = [], [], []
    for i, (a, b) in enumerate(zip(starts, ends)):
        a, b = int(a), int(b)
        if b <= a:
            continue
        w = b - a if window == 0 else int(window)
        for x in range(a, b, w):
            seg.append(i)
            s.append(x)
            e.append(min(x + w, b))
    return np.array(seg, np.int64), np.array(s, np.int64), np.array(e, np.int64)
