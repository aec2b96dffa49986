"""Per-position base counts on the GPU (csrc/bases.hip) against the model in
tests/bases_model.py: exact equality of seg_off, the six planes and the sites.
Shapes are a few tiles at most; P (tile positions) comes from the library."""
import ctypes
import os
import re

import numpy as np
import pytest
from click.testing import CliRunner

from metacov_amd import _lib
from metacov_amd import bases as mb
from tests import bases_model as bm
from tests.bases_model import A, C, G, T, N, DEL

pytestmark = pytest.mark.gpu

ALL_OPS = "2H3S5M2I4M3D6M7N2=1X1P2M4S"
N_REF = 4


@pytest.fixture(scope="module")
def bc(lib_built):
    h = mb.BaseCounter(N_REF, 0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def P(lib_built):
    return mb.dims()


def letters(rng, n):
    return "".join(rng.choice(list("ACGTN"), size=n, p=[.24, .24, .24, .24, .04]))


def read(rng, tid, pos, cigar, quals=30):
    n = bm.query_length(bm.cigar_words(cigar))
    return (tid, pos, cigar, letters(rng, n), quals)


def run(bc, batches, segs, min_baseq=0):
    if isinstance(batches, dict):
        batches = [batches]
    tids, starts, ends = (np.array(x, np.int64) for x in zip(*segs)) if segs else (np.zeros(0, np.int64),) * 3
    n = bc.begin(tids, starts, ends, min_baseq=min_baseq)
    for b in batches:
        bc.add_reads(*bm.batch_args(b))
    got = bc.counts()
    assert got.dtype == np.uint32 and got.shape == (6, n)
    return tids, starts, ends, bc.seg_off, got


def check(bc, batches, segs, min_baseq=0):
    tids, starts, ends, off, got = run(bc, batches, segs, min_baseq)
    want_off, want = bm.counts_model(batches, tids, starts, ends, min_baseq)
    assert np.array_equal(off, want_off)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "first difference at (channel, index) %s: got %d, want %d" % (
        bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    return got


def batch(reads, **kw):
    return bm.make_batch(sorted(reads, key=lambda r: (r[0], r[1])), **kw)


# ------------------------------------------------------------------ CIGAR ops

def test_cigar_ops(bc):
    rng = np.random.default_rng(1)
    reads = [read(rng, 0, 5 + 40 * k, c) for k, c in enumerate(
        ["9M", "4M3I5M", "4M3D5M", "4M9N5M", "3S6M", "6M3S", "2H6M2H", "4M2P4M", "8=", "8X", "3=2X3=",
         ALL_OPS, "1M", "1D", "5I"])]
    got = check(bc, batch(reads), [(0, 0, 700)])
    assert got[DEL].sum() == 3 + 3 + 1 and got.sum() > 0
    # by hand: the all-ops read (test_bases.test_model_by_hand's), at odd arena offsets
    bases = "NNNACGTNAAACGTCCCCCCGTANNNNGG"
    got = check(bc, bm.make_batch([(1, 10, ALL_OPS, bases, 30)], seq_gap=1, qual_gap=3), [(1, 0, 50)])
    assert got[:, 10:15].argmax(axis=0).tolist() == [A, C, G, T, N]
    assert got[DEL, 19:22].tolist() == [1, 1, 1] and got[:, 28:35].sum() == 0
    assert got[:, 35:40].argmax(axis=0).tolist() == [G, T, A, N, N] and got.sum() == 5 + 4 + 3 + 6 + 2 + 1 + 2


def test_channel_table(bc):
    got = check(bc, bm.make_batch([(0, 3, "16M", list(range(16)), 30)]), [(0, 0, 20)])
    assert got[:, 3:19].argmax(axis=0).tolist() == [N, A, C, N, G, N, N, N, T] + [N] * 7


@pytest.mark.parametrize("gap", [0, 1])
def test_nibble_alignment(bc, gap):
    """Odd and even l_seq, reads at odd and even byte offsets, distinct first
    and last bases."""
    reads = []
    for k, n in enumerate([1, 2, 3, 4, 5, 64, 65, 127, 128, 129]):
        s = "C" + "A" * (n - 2) + "G" if n > 1 else "T"
        reads.append((0, 10 + 150 * k, "%dM" % n, s, list(range(n))))
    got = check(bc, bm.make_batch(reads, seq_gap=gap, qual_gap=gap), [(0, 0, 1600)])
    assert got[C, 10 + 150 * 4] == 1 and got[G, 10 + 150 * 4 + 4] == 1 and got[T, 10] == 1


# ----------------------------------------------------------------- tile edges

def test_tile_edges(bc, P):
    rng = np.random.default_rng(2)
    lens = [1, P - 1, P, P + 1, 2 * P + 1]
    n_ref = len(lens)
    with mb.BaseCounter(n_ref, 0) as h:
        reads = []
        for t, L in enumerate(lens):
            reads.append(read(rng, t, 0, "1M"))
            reads.append(read(rng, t, L - 1, "1M"))
            if L > 200:
                reads += [read(rng, t, L - 100, "100M"), read(rng, t, L - 50, "100M"),      # ends at / overhangs L
                          read(rng, t, 0, "60M")]
        # on the longest: M and D straddling P, an I exactly at P, reads ending at P, starting at P - 1
        reads += [read(rng, 4, P - 30, "60M"), read(rng, 4, P - 20, "15M10D15M"), read(rng, 4, P - 10, "10M5I10M"),
                  read(rng, 4, P - 40, "40M"), read(rng, 4, P - 1, "40M"), read(rng, 4, P - 1, "1M"),
                  read(rng, 4, P, "1M"), read(rng, 4, 2 * P - 7, "7M3D1M")]
        check(h, batch(reads), [(t, 0, L) for t, L in enumerate(lens)])


def test_halo(bc, P):
    rng = np.random.default_rng(3)
    long_span = 3 * P + 5
    reads = [read(rng, 0, 17, "%dM" % long_span)]                       # one long read among short ones
    reads += [read(rng, 0, int(p), "40M") for p in rng.integers(0, 5 * P, size=60)]
    # max_span = 3P + 5: a read of that span ending exactly at 4P (does not reach tile 4) and one whose
    # last base alone reaches it
    reads += [read(rng, 0, P - 5, "%dM" % long_span), read(rng, 0, P - 4, "%dM" % long_span)]
    check(bc, batch(reads), [(0, 0, 5 * P + 100)])
    # more than 64 ops, and one op longer than 2P
    many = "".join(["3M1I2M1D"] * 40) + "5M"
    reads = [read(rng, 1, P - 100, many), read(rng, 1, 50, "10M%dD10M" % (2 * P + 9)),
             read(rng, 1, 60, "10M%dN10M" % (2 * P + 9)), read(rng, 1, 70, "%d=" % (2 * P + 3))]
    assert len(bm.cigar_words(many)) > 64
    got = check(bc, batch(reads), [(1, 0, 3 * P)])
    assert got[DEL].sum() == 40 + 2 * P + 9


def test_deep_pile(bc):
    """70 000 one-base reads on one position (more than 16 bits) next to an
    empty one."""
    n, n_a = 70000, 40000
    b = {"tid": np.zeros(n, np.int32), "pos": np.full(n, 7, np.int32), "l_seq": np.ones(n, np.int32),
         "cig_off": np.arange(n + 1, dtype=np.int64), "cigar": np.full(n, (1 << 4) | 0, np.uint32),
         "seq_off": np.arange(n + 1, dtype=np.int64),
         "seq": np.where(np.arange(n) < n_a, 0x10, 0x20).astype(np.uint8),
         "qual_off": np.arange(n + 1, dtype=np.int64), "qual": np.full(n, 30, np.uint8)}
    _, _, _, _, got = run(bc, b, [(0, 0, 16)])
    want = np.zeros((6, 16), np.uint32)
    want[A, 7], want[C, 7] = n_a, n - n_a
    assert np.array_equal(got, want)


# ------------------------------------------------------------------- segments

def test_segments(bc, P):
    rng = np.random.default_rng(4)
    L = P + 300                                                   # the contig "ends" at L; a read overhangs it
    reads = [read(rng, 1, int(p), "50M2D48M") for p in rng.integers(0, L - 100, size=80)]
    reads += [read(rng, 1, L - 30, "80M"), read(rng, 0, 3, "20M"), read(rng, 2, 0, "9M")]
    segs = [(1, 1, 50), (1, 2, P + 3), (1, 3, L), (1, 5, 6), (1, P - 1, P + 1), (1, P, P + 2),
            (1, 7, L - 5), (1, 9, L + 100), (1, L - 1, L + 1), (1, L, L + 9), (1, L + 40, L + 2 * P),
            (1, L + 60, L + 70),                                  # wholly past the last read
            (1, 10, 10), (1, L + 3, L + 3), (0, 0, 0),            # empty
            (0, 1, 3), (0, 0, 50), (1, 2, P + 3), (1, 2, P + 3),  # duplicates
            (2, 0, 9), (3, 0, 100)]
    got = check(bc, batch(reads), segs)
    assert got.sum() > 0
    order = np.random.default_rng(5).permutation(len(segs))
    check(bc, batch(reads), [segs[i] for i in order])
    check(bc, batch(reads), [])


@pytest.mark.parametrize("bad", [([4], [0], [5]), ([-1], [0], [5]), ([0], [-1], [5]), ([0], [6], [5]),
                                 ([0], [0], [(1 << 40) + 1])])
def test_bad_segments(bc, bad):
    with pytest.raises(_lib.MetacovError, match="segment 0") as e:
        bc.begin(*bad)
    assert e.value.code == _lib.MC_E_INVALID
    with pytest.raises(_lib.MetacovError) as e:                 # a failed begin leaves no segments
        bc.counts(0, 0)
    assert e.value.code == _lib.MC_E_STATE
    check(bc, bm.make_batch([(0, 1, "3M", "ACG", 30)]), [(0, 0, 5)])


# ------------------------------------------------------------------ min_baseq

@pytest.mark.parametrize("mq", [0, 15, 41])
def test_min_baseq(bc, mq):
    reads = [(0, 0, "5M2D5M", "ACGTACGTAC", [14, 15, 16, 40, 41, 42, 0, 255, 15, 41]),
             (0, 2, "6M", "TTTTTT", None),                        # qualities absent: passes any threshold
             (0, 3, "2S4M", "GGCCCC", [0, 0, 41, 41, 40, 15]),
             (0, 4, "3M", "AAA", [255, 0, 0])]                    # first byte 0xFF: absent too
    got = check(bc, bm.make_batch(reads), [(0, 0, 16)], mq)
    assert got[DEL, 5:7].tolist() == [1, 1]                       # DEL unaffected
    assert got[T, 2] == 1 and got[T, 3] == (2 if mq <= 40 else 1) # the read without qualities always counts
    assert got[C, 5] == (1 if mq <= 40 else 0) and got[C, 6] == (1 if mq <= 15 else 0)
    assert got[C, 1] == (1 if mq <= 15 else 0)                    # quality exactly 15
    assert got[A, 4] == (2 if mq <= 41 else 1)                    # read 0's Q41 A at 4, read 3's absent A


# ------------------------------------------------------------------- batching

def test_batching_and_reuse(bc, P):
    rng = np.random.default_rng(6)
    reads = [read(rng, 0, int(p), "30M1D30M") for p in rng.integers(P - 200, P + 200, size=90)]
    reads += [read(rng, 0, P - 3, "6M") for _ in range(30)]                   # a pile on the tile edge
    b = batch(reads)
    n = bm.n_reads(b)
    segs = [(0, 0, 2 * P + 50), (0, P - 10, P + 10)]
    one = check(bc, b, segs).copy()
    k1 = int(np.searchsorted(b["pos"], P - 3)) + 10                           # cuts inside the pile
    k2 = k1 + 15
    assert b["pos"][k1 - 1] == b["pos"][k1] == b["pos"][k2] == P - 3
    three = check(bc, [bm.slice_batch(b, 0, k1), bm.slice_batch(b, k1, k2), bm.slice_batch(b, k2, n)], segs)
    assert np.array_equal(one, three)
    # begin twice: the second starts from zero
    bc.begin([0], [0], [100])
    bc.add_reads(*bm.batch_args(bm.make_batch([(0, 5, "4M", "ACGT", 30)])))
    assert bc.counts().sum() == 4
    bc.begin([0], [0], [100])
    assert bc.counts().sum() == 0
    # a smaller and a larger N on the same handle
    check(bc, b, [(0, P - 5, P + 5)])
    check(bc, b, [(0, 0, 6 * P + 1), (0, 0, P)])
    assert np.array_equal(check(bc, b, segs), one)
    # an empty batch adds nothing; batches must stay sorted across calls
    bc.add_reads(*bm.batch_args(bm.make_batch([])))
    with pytest.raises(_lib.MetacovError, match="previous batch"):
        bc.add_reads(*bm.batch_args(bm.make_batch([(0, 0, "1M", "A", 30)])))
    assert np.array_equal(bc.counts(), one)


# --------------------------------------------------------------------- errors

def test_invalid_batches(bc):
    rng = np.random.default_rng(7)
    good = [read(rng, 0, 10 * k, "12M") for k in range(300)]
    segs = [(0, 0, 3100)]

    def expect(reads, match, **kw):
        bc.begin([0], [0], [3100])
        with pytest.raises(_lib.MetacovError, match=match) as e:
            bc.add_reads(*bm.batch_args(bm.make_batch(reads, **kw)))
        assert e.value.code == _lib.MC_E_INVALID
        assert bc.counts().sum() == 0                             # the batch added nothing
        check(bc, bm.make_batch(good), segs)                      # and the handle is usable

    r = list(good)
    r[200], r[201] = r[201], r[200]
    expect(r, "read 201: .*not sorted")
    r = list(good)
    r[259] = (N_REF,) + r[259][1:]
    expect(r[:260], "read 259: tid %d out of range" % N_REF)
    r = list(good)
    r[0] = (-1,) + r[0][1:]
    expect(r, "read 0: tid -1 out of range")
    r = list(good)
    r[0] = (0, -5) + r[0][2:]
    expect(r, "read 0: negative pos")
    ls = [12] * 300
    ls[77], ls[130] = 11, 13
    expect(good, "read 77: CIGAR query length 12 differs from l_seq 11", l_seq=ls)
    r = list(good)
    r[299] = (0, 2990, "".join(["1M%dN" % ((1 << 28) - 1)] * 8) + "4M", r[299][3], 30)
    expect(r, "read 299: reference span")


def test_invalid_batches_device(bc):
    """test_invalid_batches' batches through mc_bases_add_batch_device, the
    arrays uploaded with torch: code and message are the host entry point's,
    the planes stay zero and the handle takes the good batch afterwards.  Then
    a batch that starts before the previous one ended, on both paths: that
    message comes before the verdict on a bad read further in."""
    import torch
    lib = bc._lib
    rng = np.random.default_rng(7)
    good = [read(rng, 0, 10 * k, "12M") for k in range(300)]
    tids, starts, ends = np.array([0]), np.array([0]), np.array([3100])
    gb = bm.make_batch(good)
    _, want = bm.counts_model([gb], tids, starts, ends, 0)

    def host(b):
        rc = lib.mc_bases_add_batch(bc._h, bm.n_reads(b), *[_lib.ptr(a) for a in bm.batch_args(b)])
        return rc, lib.mc_last_error().decode() if rc else ""

    def device(b):
        arrs = bm.batch_args(b)
        dev = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for a in arrs]
        torch.cuda.synchronize()
        tid, pos, cig_off, cigar, l_seq, seq_off, seq, qual_off, qual = [ctypes.c_void_p(t.data_ptr()) for t in dev]
        rc = lib.mc_bases_add_batch_device(bc._h, bm.n_reads(b), tid, pos, cig_off, cigar, len(b["cigar"]), l_seq,
                                           seq_off, seq, len(b["seq"]), qual_off, qual, len(b["qual"]))
        return rc, lib.mc_last_error().decode() if rc else ""

    def expect(reads, match, **kw):
        b = bm.make_batch(reads, **kw)
        bc.begin(tids, starts, ends)
        rc, msg = host(b)
        assert rc == _lib.MC_E_INVALID and re.search(match, msg), msg
        bc.begin(tids, starts, ends)
        assert device(b) == (rc, msg)
        assert bc.counts().sum() == 0                             # the batch added nothing
        assert device(gb) == (_lib.MC_OK, "")                     # and the handle is usable
        assert np.array_equal(bc.counts(), want)

    r = list(good)
    r[200], r[201] = r[201], r[200]
    expect(r, "^read 201: .*not sorted")
    r = list(good)
    r[259] = (N_REF,) + r[259][1:]
    expect(r[:260], "^read 259: tid %d out of range" % N_REF)
    r = list(good)
    r[0] = (-1,) + r[0][1:]
    expect(r, "^read 0: tid -1 out of range")
    r = list(good)
    r[0] = (0, -5) + r[0][2:]
    expect(r, "^read 0: negative pos")
    ls = [12] * 300
    ls[77], ls[130] = 11, 13
    expect(good, "^read 77: CIGAR query length 12 differs from l_seq 11", l_seq=ls)
    r = list(good)
    r[299] = (0, 2990, "".join(["1M%dN" % ((1 << 28) - 1)] * 8) + "4M", r[299][3], 30)
    expect(r, "^read 299: reference span")
    # the previous batch ended at 2990
    early = bm.make_batch([(0, 2989, "1M", "A", 30), (0, 2995, "1M", "A", 30), (0, 2994, "1M", "A", 30)])
    seen = []
    for add in (host, device):
        bc.begin(tids, starts, ends)
        assert add(gb) == (_lib.MC_OK, "")
        seen.append(add(early))
        assert np.array_equal(bc.counts(), want)
        assert add(bm.slice_batch(early, 1, 2)) == (_lib.MC_OK, "")          # 2995 alone follows 2990
        assert bc.counts().sum() == want.sum() + 1
    assert seen[0] == seen[1] == (_lib.MC_E_INVALID,
                                  "read 0: reads are not sorted by (tid, pos) against the previous batch")


def test_calls_out_of_order(lib_built):
    with mb.BaseCounter(2, 0) as h:
        b = bm.make_batch([(0, 0, "1M", "A", 30)])
        for call in (lambda: h.add_reads(*bm.batch_args(b)), lambda: h.sites(), lambda: h.counts(0, 0),
                     lambda: h.timing()):
            with pytest.raises(_lib.MetacovError) as e:
                call()
            assert e.value.code == _lib.MC_E_STATE
        h.begin([1], [0], [4])
        h.add_reads(*bm.batch_args(bm.make_batch([(1, 1, "2M", "CG", 30)])))
        assert h.counts().tolist() == [[0] * 4, [0, 1, 0, 0], [0, 0, 1, 0], [0] * 4, [0] * 4, [0] * 4]
        with pytest.raises(_lib.MetacovError) as e:
            h.counts(3, 2)
        assert e.value.code == _lib.MC_E_INVALID
        for bad in ((-1, 1, 0), (1, -1, 0), (1, 1, -1), (1, 1, 1000001)):
            with pytest.raises(_lib.MetacovError) as e:
                h.sites(*bad)
            assert e.value.code == _lib.MC_E_INVALID
        assert len(h.sites(1, 0, 0)) == 2
        t = h.timing()
        assert t["reads"] == 1 and t["tiles"] == 1 and t["pileup_ms"] > 0


# ---------------------------------------------------------------------- sites

def pile(cols, tid=0, start=0):
    """Reads that give position start + i the six counts cols[i]."""
    reads = []
    for i, col in enumerate(cols):
        for ch, k in enumerate(col):
            for _ in range(int(k)):
                reads.append((tid, start + i, "1D", "", 30) if ch == DEL else (tid, start + i, "1M", "ACGTN"[ch], 30))
    return bm.make_batch(reads)


def check_sites(bc, planes, starts, args, ref=None):
    got = bc.sites(*args, ref=ref)
    first, pos, cnt = bm.sites_model(planes, bc.seg_off, starts, *args, ref=ref)
    assert got.first.dtype == np.int64 and got.pos.dtype == np.int64 and got.counts.dtype == np.uint32
    assert np.array_equal(got.first, first) and np.array_equal(got.pos, pos) and np.array_equal(got.counts, cnt)
    return got


def test_sites_thresholds(bc):
    #          A  C  G  T  N DEL
    cols = [(7, 1, 0, 0, 0, 0),      # 0: alt 1 of 8 = 125 000 ppm exactly
            (4, 3, 0, 0, 2, 0),      # 1: alt 3 of 7 = 428 571.43 ppm; N is no allele
            (5, 5, 0, 0, 0, 0),      # 2: tie A = C: base A, alt 5
            (0, 2, 2, 2, 0, 0),      # 3: three-way tie: base C, alt 2
            (0, 0, 0, 6, 0, 2),      # 4: alt = DEL
            (0, 3, 0, 0, 0, 0),      # 5: major allele C, no minor allele
            (0, 0, 0, 0, 4, 0),      # 6: only N: depth 0
            (0, 0, 0, 0, 0, 0),      # 7: empty
            (0, 0, 0, 0, 0, 3)]      # 8: only DEL
    planes = check(bc, pile(cols, start=20), [(0, 20, 29)])
    assert np.array_equal(planes.T, np.array(cols))
    st = [20]
    assert check_sites(bc, planes, st, (1, 1, 0)).pos.tolist() == [20, 21, 22, 23, 24]
    assert check_sites(bc, planes, st, (1, 2, 0)).pos.tolist() == [21, 22, 23, 24]      # alt == min_count at 23, 24
    assert check_sites(bc, planes, st, (1, 3, 0)).pos.tolist() == [21, 22]              # min_count - 1 there
    assert check_sites(bc, planes, st, (1, 1, 125000)).pos.tolist() == [20, 21, 22, 23, 24]
    assert check_sites(bc, planes, st, (1, 1, 125001)).pos.tolist() == [21, 22, 23, 24]
    assert check_sites(bc, planes, st, (1, 1, 428571)).pos.tolist() == [21, 22]
    assert check_sites(bc, planes, st, (1, 1, 428572)).pos.tolist() == [22]
    assert check_sites(bc, planes, st, (1, 1, 500000)).pos.tolist() == [22]
    assert check_sites(bc, planes, st, (1, 1, 500001)).pos.tolist() == []               # zero sites
    assert check_sites(bc, planes, st, (9, 1, 0)).pos.tolist() == [22]                  # depth 10 only
    assert check_sites(bc, planes, st, (0, 0, 0)).pos.tolist() == list(range(20, 29))   # every position
    # with a reference plane: 5 (only C) against ref A is a site although it has no minor allele; ref
    # code 4 falls back to the major allele; at 2 the reference T makes alt = 5 either way
    ref = np.array([0, 0, 3, 4, 3, 0, 0, 4, 4], np.uint8)
    assert check_sites(bc, planes, st, (1, 1, 0), ref).pos.tolist() == [20, 21, 22, 23, 24, 25]
    assert check_sites(bc, planes, st, (1, 3, 0), ref).pos.tolist() == [21, 22, 25]
    ref[5] = 1
    assert check_sites(bc, planes, st, (1, 1, 0), ref).pos.tolist() == [20, 21, 22, 23, 24]
    ref[0] = 1                                                                          # ref C at 0: alt = A = 7
    assert check_sites(bc, planes, st, (1, 7, 0), ref).pos.tolist() == [20]


def test_sites_tiles_and_segments(bc, P):
    rng = np.random.default_rng(8)
    L = 2 * P + 1
    reads = [read(rng, 0, int(p), "70M") for p in rng.integers(0, L - 70, size=400)]
    reads += [(0, P - 1, "2M", "AC", 30)] * 3 + [(0, P - 1, "2M", "GT", 30)] * 2          # sites at P - 1 and P
    segs = [(0, 0, L), (0, 5, 5), (0, P - 1, P + 1), (1, 0, 10), (0, P - 300, L + 40), (0, 0, 0)]
    planes = check(bc, batch(reads), segs)
    starts = [s[1] for s in segs]
    got = check_sites(bc, planes, starts, (1, 1, 0))
    assert {P - 1, P} <= set(got.pos[got.first[0]:got.first[1]].tolist())
    assert got.pos[got.first[2]:got.first[3]].tolist() == [P - 1, P]
    assert got.first[1] == got.first[2] and got.first[3] == got.first[4]
    check_sites(bc, planes, starts, (3, 2, 100000))
    every = check_sites(bc, planes, starts, (0, 0, 0))
    assert len(every) == planes.shape[1]
    assert len(check_sites(bc, planes, starts, (1 << 40, 0, 0))) == 0
    ref = rng.integers(0, 5, size=planes.shape[1]).astype(np.uint8)
    check_sites(bc, planes, starts, (1, 1, 0), ref)
    check_sites(bc, planes, starts, (2, 2, 250000), ref)


def test_sites_many_one_position_segments(bc):
    """5000 segments of one position each: more tiles than one scan iteration
    (4096).  The tiles on both sides of that edge are sites, are none, and are
    mixed; thresholds that keep no position and every position besides."""
    rng = np.random.default_rng(21)
    S, edge = 5000, slice(4094, 4098)
    segs = [(int(rng.integers(0, N_REF)), i, i + 1) for i in rng.integers(0, 10 ** 6, size=S).tolist()]
    tids, starts, ends = (np.array(x, np.int64) for x in zip(*segs))
    assert bc.begin(tids, starts, ends) == S
    assert bc.timing()["tiles"] == S
    args = (10, 3, 100000)
    col = {1: (30, 9, 0, 0, 2, 0),           # C: 9 of 39 beside the base allele A
           0: (30, 2, 0, 0, 9, 0)}           # C: 2 < min_count; N is no allele
    ref = rng.integers(0, 5, size=S).astype(np.uint8)
    ref[edge] = [0, 4, 0, 4]                 # A, or unknown: the major allele A
    for pattern in ((1, 1, 1, 1), (0, 0, 0, 0), (1, 0, 0, 1), (0, 1, 1, 0)):
        planes = rng.integers(0, 25, size=(6, S)).astype(np.uint32)
        planes[:, rng.random(S) < 0.2] = 0
        planes[:, edge] = np.array([col[k] for k in pattern], np.uint32).T
        bc.set_counts(0, planes)
        for r in (None, ref):
            got = check_sites(bc, planes, starts, args, r)
            assert 0 < len(got) < S
            assert np.diff(got.first)[edge].tolist() == list(pattern)
        assert len(check_sites(bc, planes, starts, (1 << 40, 0, 0))) == 0
        assert len(check_sites(bc, planes, starts, (0, 0, 0), ref)) == S


# ------------------------------------------------------------ the int32 edge

def test_int32_edge(bc, P):
    """Positions around 2^31 and reference ends below 2^32
    (bases_model.int32_edge_case): the planes, seg_off and the sites with
    their int64 positions, with the segments in two orders and the reads in
    one batch and in two."""
    H = 1 << 31
    rng = np.random.default_rng(9)
    reads, segs, scrambled, k = bm.int32_edge_case(P)
    b = bm.make_batch(reads)
    n = bm.n_reads(b)
    assert int(b["pos"].max()) == H - 1 and b["pos"][k - 1] < H - P <= b["pos"][k] and b["tid"][k] == 1
    for sg in (segs, scrambled):
        planes = check(bc, b, sg).copy()
        starts = [s[1] for s in sg]
        for s in range(len(sg)):                                          # every segment holds counts
            assert planes[:, bc.seg_off[s]:bc.seg_off[s + 1]].sum() > 0, sg[s]
        got = check_sites(bc, planes, starts, (1, 1, 0))
        assert got.pos.max() > H + (1 << 30) and (got.pos == H - 1).sum() >= 2 and (got.pos == H).sum() == 1
        assert (got.pos < 400).any()
        every = check_sites(bc, planes, starts, (0, 0, 0))
        assert np.array_equal(every.pos, np.concatenate([np.arange(x, y, dtype=np.int64) for _, x, y in sg]))
        ref = rng.integers(0, 5, size=planes.shape[1]).astype(np.uint8)
        check_sites(bc, planes, starts, (1, 1, 0), ref)
        check_sites(bc, planes, starts, (2, 2, 200000), ref)
        two = check(bc, [bm.slice_batch(b, 0, k), bm.slice_batch(b, k, n)], sg)
        assert np.array_equal(two, planes)
    # min_baseq, and one read per batch around 2^31: every batch has its own maximum span and tile range
    check(bc, b, segs, 31)
    a = int(np.searchsorted(b["pos"][:n - 40], H - 60))
    check(bc, [bm.slice_batch(b, 0, a)] + [bm.slice_batch(b, i, i + 1) for i in range(a, n - 40)] +
          [bm.slice_batch(b, n - 40, n)], segs)


# ----------------------------------------------------------------------- fuzz

def random_cigar(rng, P):
    ops = []
    for _ in range(int(rng.integers(1, 9))):
        op = int(rng.choice([0, 0, 0, 0, 1, 2, 2, 3, 4, 5, 6, 7, 8]))
        n = int(rng.integers(1, 400)) if rng.random() < 0.9 else int(rng.integers(P, 2 * P + 50))
        if op in (1, 4, 5, 6):
            n = int(rng.integers(1, 12))
        ops.append("%d%s" % (n, bm.OPS[op]))
    return "".join(ops)


@pytest.mark.parametrize("seed", range(20))
def test_fuzz(bc, P, seed):
    rng = np.random.default_rng(100 + seed)
    L = 3 * P + int(rng.integers(0, 50))
    reads = []
    for _ in range(int(rng.integers(20, 90))):
        c = random_cigar(rng, P)
        n = bm.query_length(bm.cigar_words(c))
        q = None if rng.random() < 0.1 else rng.integers(0, 45, size=n).tolist()
        reads.append((int(rng.integers(0, 3)), int(rng.integers(0, L)), c, rng.integers(0, 16, size=n).tolist(), q))
    segs = []
    for _ in range(int(rng.integers(1, 8))):
        a = int(rng.integers(0, L + 100))
        segs.append((int(rng.integers(0, N_REF)), a, a + int(rng.integers(0, L))))
    b = batch(reads, seq_gap=seed % 3, qual_gap=seed % 2)
    mq = [0, 15, 30, 41][seed % 4]
    if seed % 5 == 0:
        h = bm.n_reads(b) // 3
        b = [bm.slice_batch(b, 0, h), bm.slice_batch(b, h, bm.n_reads(b))]
    planes = check(bc, b, segs, mq)
    check_sites(bc, planes, [s[1] for s in segs], (int(rng.integers(0, 4)), int(rng.integers(0, 3)),
                                                    int(rng.integers(0, 400000))),
                rng.integers(0, 5, size=planes.shape[1]).astype(np.uint8) if seed % 2 else None)


# ------------------------------------------------- against the engine, end to end

@pytest.fixture(scope="module")
def bbmap(golden_dir):
    path = os.path.join(golden_dir, "bbmap.sorted.bam")
    names, lengths, b, _ = bm.kept_reads(path)
    n = len(lengths)
    planes = bm.counts_model(b, np.arange(n), np.zeros(n, np.int64), lengths)
    return path, names, lengths, b, planes


@pytest.mark.parametrize("name", ["bbmap.sorted.bam", "synth_exp.bam"])
def test_total_equals_engine_depth(lib_built, golden_dir, name):
    from metacov_amd.bam import BamFile
    path = os.path.join(golden_dir, name)
    with BamFile(path) as bam:
        eng = bam.engine(0)
        lengths = list(bam.lengths)
        with mb.BaseCounter(len(lengths), 0) as h:
            h.begin(np.arange(len(lengths)), np.zeros(len(lengths), np.int64), lengths)
            c = h.add_bam(path, max_reads=1000)                      # several batches
            assert c["no_seq"] == 0 and c["bad_cigar"] == 0
            total = h.counts().astype(np.int64).sum(axis=0)
            off = h.seg_off
        assert total.sum() > 0
        for t, L in enumerate(lengths):
            assert np.array_equal(total[off[t]:off[t + 1]], eng.depth(t, 0, L)), t


def test_add_bam_equals_model(bc, bbmap):
    path, names, lengths, b, (want_off, want) = bbmap
    with mb.BaseCounter(len(lengths), 0) as h:
        h.begin(np.arange(len(lengths)), np.zeros(len(lengths), np.int64), lengths)
        h.add_bam(path)
        assert np.array_equal(h.seg_off, want_off) and np.array_equal(h.counts(), want)
        h.begin(np.arange(len(lengths)), np.zeros(len(lengths), np.int64), lengths)
        h.add_bam(path, min_mapq=30)
        b30 = bm.kept_reads(path, min_mapq=30)[2]
        assert np.array_equal(h.counts(), bm.counts_model(b30, np.arange(len(lengths)), np.zeros(len(lengths)),
                                                          lengths)[1])


def test_cli_all_with_reference(bbmap, golden_dir, tmp_path):
    from metacov_amd.cli import main
    path, names, lengths, b, (off, planes) = bbmap
    fa = os.path.join(golden_dir, "reference_1K.fa.gz")
    out = tmp_path / "all.tsv"
    r = CliRunner().invoke(main, ["bases", "-b", path, "-f", fa, "--all", "-o", str(out)])
    assert r.exit_code == 0, r.output
    rows = [(t, p, planes[:, off[t] + p]) for t, L in enumerate(lengths) for p in range(L)]
    assert out.read_text() == bm.table(dict(enumerate(names)), rows, bm.read_fasta(fa))
    every = out.read_text()
    # the sites, against the reference and without it (the file has one site at these thresholds), and
    # thresholds of zero, which make every position a site
    seqs = bm.read_fasta(fa)
    code = np.concatenate([np.array([{"A": 0, "C": 1, "G": 2, "T": 3}.get(ch, 4) for ch in
                                     (seqs.get(names[t], "").upper() + "N" * L)[:L]], np.uint8)
                           for t, L in enumerate(lengths)])
    for ref, (d, c, frac, ppm) in ((True, (4, 2, "0.005", 5000)), (False, (4, 2, "0.005", 5000)),
                                   (True, (0, 0, "0", 0))):
        r = CliRunner().invoke(main, ["bases", "-b", path, "-o", str(out), "--min-depth", str(d), "--min-count",
                                      str(c), "--min-frac", frac] + (["-f", fa] if ref else []))
        assert r.exit_code == 0, r.output
        first, pos, cnt = bm.sites_model(planes, off, np.zeros(len(lengths), np.int64), d, c, ppm,
                                         code if ref else None)
        rows = [(t, int(pos[i]), cnt[i]) for t in range(len(lengths)) for i in range(first[t], first[t + 1])]
        assert out.read_text() == bm.table(dict(enumerate(names)), rows, seqs if ref else None)
        assert len(rows) == (sum(lengths) if ppm == 0 else 1)
        if ppm == 0:
            assert out.read_text() == every


def test_count_coverage(bbmap):
    path, names, lengths, b, _ = bbmap
    t = int(np.argmax(np.bincount(b["tid"])))
    L = lengths[t]
    _, want = bm.counts_model(b, [t], [0], [L], 15)
    got = mb.count_coverage(path, names[t], quality_threshold=15)
    assert len(got) == 4
    for g, ch in zip(got, (A, C, G, T)):
        assert g.dtype == np.uint32 and np.array_equal(g, want[ch])
    _, want = bm.counts_model(b, [t], [10], [L // 2], 0)
    got = mb.count_coverage(path, names[t], 10, L // 2, quality_threshold=0)
    assert all(np.array_equal(g, want[ch]) for g, ch in zip(got, (A, C, G, T)))
    assert not np.array_equal(want[A], bm.counts_model(b, [t], [10], [L // 2], 15)[1][A])      # Q15 discriminates
    with pytest.raises(KeyError):
        mb.count_coverage(path, "no_such_contig")
