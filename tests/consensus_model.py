"""Model of the consensus call (include/metacov_amd.h, "Consensus"), pure
Python / numpy, restated from the contract and not from the library's code:

counts     a[0..3] = A C G T, d = DEL of planes [6, N]; the N plane is ignored
depth      a0 + a1 + a2 + a3 + d
qualifies  x >= max(min_count, 1) and x * 10^6 >= call_ppm * depth
LOW        depth < max(min_depth, 1): 'N', or with fill_ref and a known
           reference code the reference base in lower case
top        the first maximum of (A, C, G, T, DEL) in channel order
DEL        top is DEL and qualifies: '-' aligned, nothing compact;
           top is DEL and does not qualify: NOCALL 'N'
base       without iupac: CALLED if top qualifies, else NOCALL 'N'
           with iupac: Q = qualifying bases; empty NOCALL, one CALLED, more
           AMBIG with ".ACMGRSVTWYHKDBN"[mask], A = 1, C = 2, G = 4, T = 8
summary    per segment: positions called ambiguous nocall low deleted differs
           length; differs = reference known and (DEL, or CALLED with another
           letter); length = positions - deleted

Counts up to 2^32 - 1 in all five channels keep every product below 2^63.
"""
import numpy as np

A, C, G, T, N, DEL = range(6)
LOW, DELETED, NOCALL, CALLED, AMBIG = range(5)
POSITIONS, COL_CALLED, COL_AMBIG, COL_NOCALL, COL_LOW, COL_DELETED, COL_DIFFERS, COL_LENGTH = range(8)
IUPAC = ".ACMGRSVTWYHKDBN"
SUMMARY_HEADER = "contig\tstart\tend\tpositions\tcalled\tambiguous\tnocall\tlow\tdeleted\tdiffers\tlength\n"


def call_loop(planes, min_depth=1, min_count=1, call_ppm=0, iupac=False, fill_ref=False, ref=None):
    """(letters uint8 [N], class int64 [N], differs bool [N]) by a literal
    per-position loop over Python integers."""
    planes = np.asarray(planes)
    n = planes.shape[1]
    letters, cls, differs = np.zeros(n, np.uint8), np.zeros(n, np.int64), np.zeros(n, bool)
    for i in range(n):
        a = [int(planes[ch, i]) for ch in (A, C, G, T)]
        d = int(planes[DEL, i])
        depth = sum(a) + d
        r = int(ref[i]) if ref is not None else 4
        known = 0 <= r <= 3

        def qualifies(x):
            return x >= max(min_count, 1) and x * 10 ** 6 >= call_ppm * depth

        if depth < max(min_depth, 1):
            k, ch = LOW, ("acgt"[r] if fill_ref and known else "N")
        else:
            five = a + [d]
            top = 0
            for j in range(1, 5):
                if five[j] > five[top]:
                    top = j
            if top == 4:
                k, ch = (DELETED, "-") if qualifies(d) else (NOCALL, "N")
            elif not iupac:
                k, ch = (CALLED, "ACGT"[top]) if qualifies(a[top]) else (NOCALL, "N")
            else:
                mask = sum(1 << b for b in range(4) if qualifies(a[b]))
                nq = bin(mask).count("1")
                if nq == 0:
                    k, ch = NOCALL, "N"
                elif nq == 1:
                    k, ch = CALLED, IUPAC[mask]
                else:
                    k, ch = AMBIG, IUPAC[mask]
        letters[i], cls[i] = ord(ch), k
        differs[i] = known and (k == DELETED or (k == CALLED and ch != "ACGT"[r]))
    return letters, cls, differs


def call(planes, min_depth=1, min_count=1, call_ppm=0, iupac=False, fill_ref=False, ref=None):
    """The same, vectorised in int64."""
    planes = np.asarray(planes)
    n = planes.shape[1]
    five = planes[[A, C, G, T, DEL]].astype(np.int64)
    depth = five.sum(axis=0)
    r = np.full(n, 4, np.int64) if ref is None else np.asarray(ref, np.int64)
    known = (r >= 0) & (r <= 3)
    rk = np.where(known, r, 0)
    q = (five >= max(min_count, 1)) & (five * 1000000 >= call_ppm * depth)          # [5, N]
    top = np.argmax(five, axis=0) if n else np.zeros(0, np.int64)                   # the first maximum
    low = depth < max(min_depth, 1)
    top_q = q[top, np.arange(n)] if n else np.zeros(0, bool)
    mask = (q[:4] * np.array([1, 2, 4, 8])[:, None]).sum(axis=0)
    if not iupac:
        mask = np.where(top < 4, mask & (1 << np.minimum(top, 3)), 0)
    nq = np.array([bin(m).count("1") for m in range(16)])[mask]
    table = np.frombuffer(IUPAC.encode(), np.uint8)
    cls = np.where(low, LOW,
                   np.where(top == 4, np.where(top_q, DELETED, NOCALL),
                            np.where(nq == 0, NOCALL, np.where(nq == 1, CALLED, AMBIG))))
    letters = np.full(n, ord("N"), np.uint8)
    base = (cls == CALLED) | (cls == AMBIG)
    letters[base] = table[mask[base]]
    letters[cls == DELETED] = ord("-")
    if fill_ref:
        fill = low & known
        letters[fill] = np.frombuffer(b"acgt", np.uint8)[rk[fill]]
    ref_letter = np.frombuffer(b"ACGT", np.uint8)[rk]
    differs = known & ((cls == DELETED) | ((cls == CALLED) & (letters != ref_letter)))
    return letters, cls, differs


def consensus_model(planes, seg_off, **kw):
    """(first int64 [S + 1], summary int64 [S, 8], aligned uint8 [N], compact
    uint8 [n_out]) of the segments seg_off [S + 1] over the planes."""
    letters, cls, differs = call(planes, **kw)
    seg_off = np.asarray(seg_off, np.int64)
    S = len(seg_off) - 1
    kept = letters != ord("-")
    first = np.zeros(S + 1, np.int64)
    summary = np.zeros((S, 8), np.int64)
    for s in range(S):
        a, b = int(seg_off[s]), int(seg_off[s + 1])
        c = cls[a:b]
        summary[s] = [b - a, (c == CALLED).sum(), (c == AMBIG).sum(), (c == NOCALL).sum(), (c == LOW).sum(),
                      (c == DELETED).sum(), differs[a:b].sum(), kept[a:b].sum()]
        first[s + 1] = first[s] + summary[s, COL_LENGTH]
    return first, summary, letters, letters[kept]


def fasta(name, letters, width=60):
    """One FASTA record as text, line by line."""
    s = bytes(np.asarray(letters, np.uint8)).decode("ascii")
    out = [">%s\n" % name]
    if width <= 0:
        if s:
            out.append(s + "\n")
    else:
        for i in range(0, len(s), width):
            out.append(s[i:i + width] + "\n")
    return "".join(out)


def summary_table(rows):
    """rows: (name, start, end, eight numbers)."""
    return SUMMARY_HEADER + "".join("%s\t%d\t%d\t%s\n" % (n, a, b, "\t".join(str(int(v)) for v in r))
                                    for n, a, b, r in rows)


# ---------------------------------------------------------- cases by hand
# (six counts A C G T N DEL, reference code or None, parameters, letter, class, differs)

M32 = 2 ** 32 - 1


def _case(cols, ref, letter, cls, differs=False, **kw):
    return (tuple(cols), ref, kw, letter, cls, differs)


HAND = [
    # LOW: no reads, only N reads; fill_ref in lower case where the reference is known
    _case((0, 0, 0, 0, 0, 0), None, "N", LOW),
    _case((0, 0, 0, 0, 5, 0), 1, "N", LOW),
    _case((0, 0, 0, 0, 0, 0), 2, "g", LOW, fill_ref=True),
    _case((0, 0, 0, 0, 0, 0), 4, "N", LOW, fill_ref=True),
    _case((1, 1, 0, 0, 0, 0), 3, "t", LOW, fill_ref=True, min_depth=3),
    _case((1, 1, 0, 0, 0, 1), 0, "A", CALLED, fill_ref=True, min_depth=3),      # depth 3 with the DEL: called
    _case((0, 0, 0, 0, 0, 0), None, "N", LOW, min_depth=0),                      # min_depth 0 acts as 1
    # CALLED, and differs against the reference
    _case((3, 0, 0, 0, 0, 0), None, "A", CALLED),
    _case((3, 0, 0, 0, 0, 0), 0, "A", CALLED, False),
    _case((3, 0, 0, 0, 0, 0), 1, "A", CALLED, True),
    _case((3, 0, 0, 0, 0, 0), 7, "A", CALLED, False),
    _case((0, 0, 0, 2, 9, 0), 3, "T", CALLED, False),
    _case((1, 0, 0, 0, 0, 0), None, "A", CALLED, min_count=0),                   # min_count 0 acts as 1
    # DEL
    _case((0, 0, 0, 0, 0, 2), 3, "-", DELETED, True),
    _case((0, 0, 0, 0, 0, 2), 4, "-", DELETED, False),
    _case((1, 0, 1, 0, 0, 2), None, "-", DELETED),
    # ties: a base against DEL, bases among themselves
    _case((2, 0, 0, 0, 0, 2), None, "A", CALLED),
    _case((0, 0, 0, 2, 0, 2), 3, "T", CALLED, False),
    _case((0, 3, 0, 3, 0, 0), None, "C", CALLED),
    _case((0, 0, 4, 4, 0, 1), 3, "G", CALLED, True),
    _case((2, 2, 2, 2, 0, 2), None, "A", CALLED),
    # DEL on top but not qualifying: no call, and no difference counted
    _case((1, 0, 0, 0, 0, 2), 0, "N", NOCALL, False, min_count=3),
    _case((2, 2, 0, 0, 0, 3), None, "N", NOCALL, call_ppm=428572),               # 3 of 7 = 428 571.43 ppm
    _case((2, 2, 0, 0, 0, 3), 1, "-", DELETED, True, call_ppm=428571),
    # thresholds at equality and one below
    _case((2, 1, 0, 0, 0, 1), None, "A", CALLED, min_depth=4),
    _case((2, 1, 0, 0, 0, 1), None, "N", LOW, min_depth=5),
    _case((3, 1, 0, 0, 0, 0), None, "A", CALLED, min_count=3),
    _case((3, 1, 0, 0, 0, 0), 1, "N", NOCALL, False, min_count=4),
    _case((7, 1, 0, 0, 0, 0), None, "A", CALLED, call_ppm=875000),               # 7 of 8 = 875 000 ppm exactly
    _case((7, 1, 0, 0, 0, 0), None, "N", NOCALL, call_ppm=875001),
    _case((1, 0, 0, 0, 0, 0), None, "A", CALLED, call_ppm=1000000),
    _case((9, 0, 0, 0, 0, 1), None, "N", NOCALL, call_ppm=1000000),
    # IUPAC beyond the 15 subsets below: unequal counts, thresholds deciding the set, DEL on top, empty set
    _case((6, 3, 0, 0, 0, 0), 0, "M", AMBIG, False, iupac=True, call_ppm=333333),
    _case((6, 3, 0, 0, 0, 0), 1, "A", CALLED, True, iupac=True, call_ppm=333334),
    _case((6, 3, 0, 0, 0, 0), None, "A", CALLED, call_ppm=333333),
    _case((0, 5, 1, 4, 0, 0), None, "Y", AMBIG, iupac=True, min_count=2),
    _case((2, 2, 0, 0, 0, 3), None, "-", DELETED, iupac=True),
    _case((2, 2, 0, 0, 0, 3), None, "N", NOCALL, iupac=True, min_count=4),       # DEL on top, below min_count
    _case((2, 2, 0, 0, 0, 1), None, "N", NOCALL, iupac=True, min_count=3),
    _case((2, 2, 0, 0, 0, 2), 2, "M", AMBIG, False, iupac=True),
    # 2^32 - 1 in every channel
    _case((M32,) * 6, 1, "A", CALLED, True),
    _case((M32,) * 6, 0, "N", AMBIG, False, iupac=True),
    _case((M32,) * 6, None, "A", CALLED, call_ppm=200000, min_depth=5 * M32),    # a fifth of the depth exactly
    _case((M32,) * 6, None, "N", NOCALL, call_ppm=200001),
    _case((M32,) * 6, None, "N", LOW, min_depth=5 * M32 + 1),
    _case((M32, 0, 0, 0, 0, M32), None, "A", CALLED, min_count=M32),
    _case((M32 - 1, 0, 0, 0, 0, M32), 0, "-", DELETED, True, min_count=M32),
]
# all 15 non-empty base subsets: 5 reads on each base of the set, with and without iupac
for _m in range(1, 16):
    _cols = tuple(5 if (_m >> b) & 1 else 0 for b in range(4)) + (0, 0)
    _single = _m & (_m - 1) == 0
    HAND.append(_case(_cols, None, IUPAC[_m], CALLED if _single else AMBIG, iupac=True))
    HAND.append(_case(_cols, None, "ACGT"[(_m & -_m).bit_length() - 1], CALLED))


def hand_groups():
    """The hand cases grouped by their parameters: [(kw, planes uint32 [6, n],
    ref uint8 [n], letters, classes, differs)]."""
    groups = {}
    for cols, ref, kw, letter, cls, differs in HAND:
        groups.setdefault(tuple(sorted(kw.items())), []).append((cols, 4 if ref is None else ref, letter, cls,
                                                                 differs))
    out = []
    for key, rows in groups.items():
        out.append((dict(key), np.array([r[0] for r in rows], np.uint32).T.copy(),
                    np.array([r[1] for r in rows], np.uint8), "".join(r[2] for r in rows),
                    [r[3] for r in rows], [r[4] for r in rows]))
    return out
