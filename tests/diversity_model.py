"""The numpy restatement of mc_bases_diversity's contract (include/metacov_amd.h,
"Diversity") on [6][N] planes, seg_off, window and ref; and a per-position
pure-Python loop that states it once more with Python integers."""
import io

import numpy as np

COLS = 8
POSITIONS, COVERED, BASES, SNV, PI_FIX, COMPARED, CON_DIFF, POP_DIFF = range(8)
MIN_WINDOW = 16
MAX_N = 1 << 26
ONE = 1 << 32


class RangeError(ValueError):
    """A covered position with 2^26 bases or more; .index is the lowest such plane index."""

    def __init__(self, index):
        super().__init__("plane index %d: 2^26 bases or more" % index)
        self.index = int(index)


def windows(seg_off, window):
    """(win_first [S + 1], seg [n], lo [n], hi [n]): the plane range of each window."""
    seg_off = np.asarray(seg_off, np.int64)
    if window != 0 and window < MIN_WINDOW:
        raise ValueError("window must be 0 or at least %d" % MIN_WINDOW)
    first, seg, lo, hi = [0], [], [], []
    for s in range(len(seg_off) - 1):
        a, b = int(seg_off[s]), int(seg_off[s + 1])
        step = window if window else max(b - a, 1)
        for x in range(a, b, step):
            seg.append(s)
            lo.append(x)
            hi.append(min(x + step, b))
        first.append(len(seg))
    return (np.array(first, np.int64), np.array(seg, np.int64), np.array(lo, np.int64), np.array(hi, np.int64))


def per_position(planes, min_depth=2, min_count=1, min_ppm=0, ref=None):
    """int64 [8, N]: each position's contribution to the columns (positions: 1)."""
    planes = np.asarray(planes)
    N = planes.shape[1]
    a = planes[:4].astype(np.int64)
    n = a.sum(axis=0)
    md, mc = max(int(min_depth), 2), max(int(min_count), 1)
    covered = n >= md
    bad = np.flatnonzero(covered & (n >= MAX_N))
    if len(bad):
        raise RangeError(bad[0])

    def qualifies(x):
        return (x >= mc) & (x * 1000000 >= int(min_ppm) * n)

    major = np.argmax(a, axis=0) if N else np.zeros(0, np.int64)        # the first maximum
    others = a.copy()
    if N:
        others[major, np.arange(N)] = -1
    minor = others.max(axis=0) if N else np.zeros(0, np.int64)
    nc = np.where(covered, n, 2)                                        # (an uncovered n may not fit the squares)
    ac = np.where(covered, a, 0)
    num = (nc * nc - (ac * ac).sum(axis=0)).astype(np.uint64)
    den = (nc * (nc - 1)).astype(np.uint64)
    q = np.rint(num.astype(np.float64) / den.astype(np.float64) * 4294967296.0).astype(np.int64)
    out = np.zeros((COLS, N), np.int64)
    out[POSITIONS] = 1
    out[COVERED] = covered
    out[BASES] = n
    out[SNV] = covered & qualifies(minor)
    out[PI_FIX] = np.where(covered, q, 0)
    if ref is not None:
        r = np.asarray(ref, np.int64)
        known = covered & (r >= 0) & (r < 4)
        ar = a[np.where(known, r, 0), np.arange(N)] if N else np.zeros(0, np.int64)
        diff = known & (major != r)
        out[COMPARED] = known
        out[CON_DIFF] = diff
        out[POP_DIFF] = diff & ~qualifies(ar)
    return out


def diversity_model(planes, seg_off, window=0, min_depth=2, min_count=1, min_ppm=0, ref=None):
    """(win_first [S + 1], rows int64 [n, 8])."""
    first, _, lo, hi = windows(seg_off, window)
    per = per_position(planes, min_depth, min_count, min_ppm, ref)
    pre = np.concatenate([np.zeros((COLS, 1), np.int64), np.cumsum(per, axis=1)], axis=1)
    rows = (pre[:, hi] - pre[:, lo]).T.reshape(-1, COLS)
    return first, np.ascontiguousarray(rows)


def position_loop(a, r, min_depth=2, min_count=1, min_ppm=0):
    """One position with Python integers: the eight contributions.  a: four
    counts; r: the reference code or None."""
    a = [int(x) for x in a]
    n = sum(a)
    md, mc = max(int(min_depth), 2), max(int(min_count), 1)
    out = [1, 0, n, 0, 0, 0, 0, 0]
    if n < md:
        return out
    if n >= MAX_N:
        raise RangeError(-1)

    def qualifies(x):
        return x >= mc and x * 10 ** 6 >= int(min_ppm) * n

    major = a.index(max(a))
    minor = max(a[:major] + a[major + 1:])
    num, den = n * n - sum(x * x for x in a), n * (n - 1)
    out[COVERED] = 1
    out[SNV] = int(qualifies(minor))
    out[PI_FIX] = int(round(float(num) / float(den) * 4294967296.0)) if num else 0    # round(): half to even
    if r is not None and 0 <= int(r) < 4:
        out[COMPARED] = 1
        if major != int(r):
            out[CON_DIFF] = 1
            out[POP_DIFF] = int(not qualifies(a[int(r)]))
    return out


def loop_model(planes, seg_off, window=0, min_depth=2, min_count=1, min_ppm=0, ref=None):
    first, _, lo, hi = windows(seg_off, window)
    planes = np.asarray(planes)
    rows = []
    for x, y in zip(lo.tolist(), hi.tolist()):
        row = [0] * COLS
        for i in range(x, y):
            c = position_loop(planes[:4, i], None if ref is None else ref[i], min_depth, min_count, min_ppm)
            row = [u + v for u, v in zip(row, c)]
        rows.append(row)
    return first, np.array(rows, np.int64).reshape(-1, COLS)


HEADER = "#contig\tstart\tend\tpositions\tcovered\tbases\tsnv\tpi\tcompared\tcon_diff\tpop_diff\tcon_ani\tpop_ani\n"


def tsv(names, starts, seg_off, window, first, rows, header=True):
    """The table `cli diversity` writes: names and starts per segment."""
    _, seg, lo, hi = windows(seg_off, window)
    fh = io.StringIO()
    if header:
        fh.write(HEADER)
    for k, row in enumerate(np.asarray(rows).tolist()):
        s = int(seg[k])
        a = int(starts[s]) + int(lo[k]) - int(seg_off[s])
        pi = "%.6f" % (row[PI_FIX] / 4294967296.0 / row[COVERED]) if row[COVERED] else "NA"
        con = "%.6f" % (1.0 - row[CON_DIFF] / row[COMPARED]) if row[COMPARED] else "NA"
        pop = "%.6f" % (1.0 - row[POP_DIFF] / row[COMPARED]) if row[COMPARED] else "NA"
        fh.write("\t".join([names[s], str(a), str(a + row[POSITIONS])] + [str(row[c]) for c in (0, 1, 2, 3)] + [pi] +
                           [str(row[c]) for c in (5, 6, 7)] + [con, pop]) + "\n")
    return fh.getvalue()
