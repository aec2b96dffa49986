"""The numpy restatement of mc_bases_compare's contract (include/metacov_amd.h,
"Comparison") on two [6][N] plane sets, seg_off and window; and a per-position
pure-Python loop that states it once more with Python integers."""
import io

import numpy as np

from tests import diversity_model as dm

COLS = 8
POSITIONS, COVERED_A, COVERED_B, COMPARED, CON_DIFF, POP_DIFF, SNV, DIST_FIX = range(8)
MAX_N = 1 << 26
ONE = 1 << 32


class RangeError(ValueError):
    """A compared position with 2^26 bases or more in a sample; .index is the lowest such plane index."""

    def __init__(self, index):
        super().__init__("plane index %d: 2^26 bases or more" % index)
        self.index = int(index)


def _sample(planes, mc, min_ppm):
    """(a int64 [4, N], n, major, minor, present bool [4, N], snv bool [N]) of one sample."""
    a = np.asarray(planes)[:4].astype(np.int64)
    N = a.shape[1]
    n = a.sum(axis=0)
    major = np.argmax(a, axis=0) if N else np.zeros(0, np.int64)        # the first maximum
    others = a.copy()
    if N:
        others[major, np.arange(N)] = -1
    minor = others.max(axis=0) if N else np.zeros(0, np.int64)

    def qualifies(x):
        return (x >= mc) & (x * 1000000 >= int(min_ppm) * n)

    present = qualifies(a) | (np.arange(4)[:, None] == major[None, :])
    return a, n, major, minor, present, qualifies(minor)


def per_position(planes_a, planes_b, min_depth=2, min_count=1, min_ppm=0):
    """int64 [8, N]: each position's contribution to the columns (positions: 1)."""
    md, mc = max(int(min_depth), 2), max(int(min_count), 1)
    a, na, major_a, _, present_a, snv_a = _sample(planes_a, mc, min_ppm)
    b, nb, major_b, _, present_b, snv_b = _sample(planes_b, mc, min_ppm)
    if a.shape != b.shape:
        raise ValueError("the two samples' planes differ in shape")
    N = a.shape[1]
    cov_a, cov_b = na >= md, nb >= md
    both = cov_a & cov_b
    bad = np.flatnonzero(both & ((na >= MAX_N) | (nb >= MAX_N)))
    if len(bad):
        raise RangeError(bad[0])
    ac, bc = np.where(both, a, 0), np.where(both, b, 0)                 # (an uncompared n may not fit the products)
    nac, nbc = np.where(both, na, 1), np.where(both, nb, 1)
    num = np.abs(ac * nbc - bc * nac).sum(axis=0).astype(np.uint64)
    den = (2 * nac * nbc).astype(np.uint64)
    q = np.rint(num.astype(np.float64) / den.astype(np.float64) * 4294967296.0).astype(np.int64)
    out = np.zeros((COLS, N), np.int64)
    out[POSITIONS] = 1
    out[COVERED_A] = cov_a
    out[COVERED_B] = cov_b
    out[COMPARED] = both
    out[CON_DIFF] = both & (major_a != major_b)
    out[POP_DIFF] = both & ~(present_a & present_b).any(axis=0)
    out[SNV] = both & (snv_a | snv_b)
    out[DIST_FIX] = np.where(both, q, 0)
    return out


def compare_model(planes_a, planes_b, seg_off, window=0, min_depth=2, min_count=1, min_ppm=0):
    """(win_first [S + 1], rows int64 [n, 8])."""
    first, _, lo, hi = dm.windows(seg_off, window)
    per = per_position(planes_a, planes_b, min_depth, min_count, min_ppm)
    pre = np.concatenate([np.zeros((COLS, 1), np.int64), np.cumsum(per, axis=1)], axis=1)
    rows = (pre[:, hi] - pre[:, lo]).T.reshape(-1, COLS)
    return first, np.ascontiguousarray(rows)


def position_loop(a, b, min_depth=2, min_count=1, min_ppm=0):
    """One position with Python integers: the eight contributions.  a, b: four counts each."""
    a, b = [int(x) for x in a], [int(x) for x in b]
    na, nb = sum(a), sum(b)
    md, mc = max(int(min_depth), 2), max(int(min_count), 1)
    out = [1, int(na >= md), int(nb >= md), 0, 0, 0, 0, 0]
    if not (out[COVERED_A] and out[COVERED_B]):
        return out
    if na >= MAX_N or nb >= MAX_N:
        raise RangeError(-1)

    def qualifies(x, n):
        return x >= mc and x * 10 ** 6 >= int(min_ppm) * n

    major_a, major_b = a.index(max(a)), b.index(max(b))
    minor_a, minor_b = max(a[:major_a] + a[major_a + 1:]), max(b[:major_b] + b[major_b + 1:])
    shared = any((c == major_a or qualifies(a[c], na)) and (c == major_b or qualifies(b[c], nb)) for c in range(4))
    num, den = sum(abs(a[c] * nb - b[c] * na) for c in range(4)), 2 * na * nb
    out[COMPARED] = 1
    out[CON_DIFF] = int(major_a != major_b)
    out[POP_DIFF] = int(not shared)
    out[SNV] = int(qualifies(minor_a, na) or qualifies(minor_b, nb))
    out[DIST_FIX] = int(round(float(num) / float(den) * 4294967296.0)) if num else 0    # round(): half to even
    return out


def loop_model(planes_a, planes_b, seg_off, window=0, min_depth=2, min_count=1, min_ppm=0):
    first, _, lo, hi = dm.windows(seg_off, window)
    planes_a, planes_b = np.asarray(planes_a), np.asarray(planes_b)
    rows = []
    for x, y in zip(lo.tolist(), hi.tolist()):
        row = [0] * COLS
        for i in range(x, y):
            c = position_loop(planes_a[:4, i], planes_b[:4, i], min_depth, min_count, min_ppm)
            row = [u + v for u, v in zip(row, c)]
        rows.append(row)
    return first, np.array(rows, np.int64).reshape(-1, COLS)


HEADER = ("#contig\tstart\tend\tpositions\tcovered_a\tcovered_b\tcompared\tcon_diff\tpop_diff\tsnv\tcon_ani\tpop_ani\t"
          "af_dist\n")


def tsv(names, starts, seg_off, window, first, rows, header=True):
    """The table `cli compare` writes: names and starts per segment."""
    _, seg, lo, hi = dm.windows(seg_off, window)
    fh = io.StringIO()
    if header:
        fh.write(HEADER)
    for k, row in enumerate(np.asarray(rows).tolist()):
        s = int(seg[k])
        a = int(starts[s]) + int(lo[k]) - int(seg_off[s])
        con = "%.6f" % (1.0 - row[CON_DIFF] / row[COMPARED]) if row[COMPARED] else "NA"
        pop = "%.6f" % (1.0 - row[POP_DIFF] / row[COMPARED]) if row[COMPARED] else "NA"
        dist = "%.6f" % (row[DIST_FIX] / 4294967296.0 / row[COMPARED]) if row[COMPARED] else "NA"
        fh.write("\t".join([names[s], str(a), str(a + row[POSITIONS])] + [str(row[c]) for c in range(7)] +
                           [con, pop, dist]) + "\n")
    return fh.getvalue()
