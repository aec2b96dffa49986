"""Model of mc_runs_compute (include/metacov_amd.h, "per-base depth as runs")
for the tests: a numpy restatement, and a deliberately naive per-position loop
to check the restatement against.

Both take the concatenated depth vector with each contig's extent and offset
(what oracle.coracle.depth returns), the segments and the quantisation edges,
and return (seg_first, start, value) as the library does."""
import numpy as np


def quantise(d, edges):
    """q(d): d itself without edges, else the number of edges <= d."""
    if edges is None or len(edges) == 0:
        return np.asarray(d, np.int64)
    return np.searchsorted(np.asarray(edges, np.int64), np.asarray(d, np.int64), side="right")


def segment_vector(depth, ext, coff, tid, start, end):
    """depth[start, end) of contig tid, zeros past the extent."""
    out = np.zeros(max(0, end - start), np.int64)
    a, b = min(start, int(ext[tid])), min(end, int(ext[tid]))
    if b > a:
        out[:b - a] = depth[coff[tid] + a:coff[tid] + b]
    return out


def runs_model(depth, ext, coff, tids, starts, ends, edges=None):
    seg_first = np.zeros(len(tids) + 1, np.int64)
    s_parts, v_parts = [], []
    for i, (t, a, b) in enumerate(zip(tids, starts, ends)):
        q = quantise(segment_vector(depth, ext, coff, int(t), int(a), int(b)), edges)
        if len(q):
            first = np.concatenate([[0], np.flatnonzero(np.diff(q) != 0) + 1])
            s_parts.append(first + int(a))
            v_parts.append(q[first])
            seg_first[i + 1] = seg_first[i] + len(first)
        else:
            seg_first[i + 1] = seg_first[i]
    start = np.concatenate(s_parts).astype(np.int64) if s_parts else np.zeros(0, np.int64)
    value = np.concatenate(v_parts).astype(np.int32) if v_parts else np.zeros(0, np.int32)
    return seg_first, start, value


def runs_loop(depth, ext, coff, tids, starts, ends, edges=None):
    """The same, one position at a time."""
    seg_first, start, value = [0], [], []
    for t, a, b in zip(tids, starts, ends):
        t, a, b = int(t), int(a), int(b)
        last = None
        for p in range(a, b):
            d = int(depth[coff[t] + p]) if p < ext[t] else 0
            if edges is not None and len(edges):
                d = sum(1 for e in edges if e <= d)
            if p == a or d != last:
                start.append(p)
                value.append(d)
            last = d
        seg_first.append(len(start))
    return (np.array(seg_first, np.int64), np.array(start, np.int64), np.array(value, np.int32))


def expand(seg_start, seg_end, start, value):
    """One segment's runs back to a vector."""
    ends = np.append(start[1:], seg_end)
    assert len(start) == 0 or start[0] == seg_start
    return np.repeat(value, ends - start)
