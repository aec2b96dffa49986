"""Consensus calling on the GPU (csrc/bases.hip: cons_call / scan / emit)
against the model in tests/consensus_model.py: exact equality of out_first,
the summary rows and both letter buffers.  Planes are set through set_counts
(mc_bases_set) except in the end-to-end tests; shapes are a few tiles at most;
P (tile positions) comes from the library."""
import ctypes
import os

import numpy as np
import pytest
from click.testing import CliRunner

from metacov_amd import _lib
from metacov_amd import bases as mb
from tests import bases_model as bm
from tests import consensus_model as cm

pytestmark = pytest.mark.gpu

N_REF = 4
DASH = ord("-")


@pytest.fixture(scope="module")
def bc(lib_built):
    h = mb.BaseCounter(N_REF, 0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def P(lib_built):
    return mb.dims()


def begin(bc, segs, planes=None):
    tids, starts, ends = (np.array(x, np.int64) for x in zip(*segs)) if segs else (np.zeros(0, np.int64),) * 3
    n = bc.begin(tids, starts, ends)
    if planes is not None:
        assert planes.shape == (6, n)
        bc.set_counts(0, planes)
        assert np.array_equal(bc.counts(), planes)
    return bc.seg_off


def random_planes(rng, n, p_del=0.2, p_empty=0.1):
    """Small counts with ties, deletion-dominated and empty positions."""
    planes = rng.integers(0, 4, size=(6, n)).astype(np.uint32)
    planes[bm.DEL] = np.where(rng.random(n) < p_del, rng.integers(3, 9, size=n), rng.integers(0, 2, size=n))
    planes[:, rng.random(n) < p_empty] = 0
    return planes


def check(bc, planes, seg_off, per_segment=40, **kw):
    """One consensus call against the model, with the per-segment invariants."""
    got = bc.consensus(**kw)
    first, summary, aligned, compact = cm.consensus_model(planes, seg_off, **kw)
    S = len(seg_off) - 1
    assert got.first.dtype == np.int64 and got.summary.dtype == np.int64 and got.summary.shape == (S, 8)
    assert np.array_equal(got.first, first)
    bad = np.argwhere(got.summary != summary)
    assert len(bad) == 0, "summary differs first at (segment, column) %s" % (bad[0],)
    assert got.n == len(compact) == int(first[-1])
    got_aligned = bc.consensus_letters(False, 0, planes.shape[1])
    got_compact = bc.consensus_letters(True, 0, got.n)
    assert got_aligned.dtype == np.uint8
    bad = np.flatnonzero(got_aligned != aligned)
    assert len(bad) == 0, "aligned differs first at %d: got %r, want %r" % (bad[0], chr(got_aligned[bad[0]]),
                                                                          chr(aligned[bad[0]]))
    assert np.array_equal(got_compact, compact)
    # invariants, per segment
    s = got.summary
    assert np.array_equal(s[:, mb.CALLED:mb.DELETED + 1].sum(axis=1), s[:, mb.POSITIONS])
    assert np.array_equal(s[:, mb.POSITIONS], np.diff(seg_off))
    assert np.array_equal(s[:, mb.LENGTH], np.diff(got.first))
    assert np.array_equal(s[:, mb.LENGTH], s[:, mb.POSITIONS] - s[:, mb.DELETED])
    for i in range(min(S, per_segment)):
        a = got.aligned(i)
        assert np.array_equal(a, aligned[seg_off[i]:seg_off[i + 1]])
        assert np.array_equal(got.compact(i), a[a != DASH])
    return got


# --------------------------------------------------------------------- rule

def test_rule_by_hand(bc):
    for kw, planes, ref, letters, classes, differs in cm.hand_groups():
        n = planes.shape[1]
        off = begin(bc, [(0, 5, 5 + n)], planes)
        got = check(bc, planes, off, ref=ref, **kw)
        assert bytes(got.aligned(0)).decode() == letters, kw
        want = [n] + [classes.count(k) for k in (cm.CALLED, cm.AMBIG, cm.NOCALL, cm.LOW, cm.DELETED)]
        assert got.summary[0, :6].tolist() == want and got.summary[0, mb.DIFFERS] == sum(differs), kw
        if not kw.get("fill_ref"):
            check(bc, planes, off, **kw)                         # and without a reference plane


def test_full_range_counts(bc, P):
    """Counts up to 2^32 - 1 in all five channels at once, over a tile edge."""
    rng = np.random.default_rng(11)
    n = P + 9
    planes = rng.integers(cm.M32 - 2, cm.M32 + 1, size=(6, n)).astype(np.uint32)
    planes[:, ::7] = cm.M32
    planes[:, 3::11] = rng.integers(0, 3, size=planes[:, 3::11].shape).astype(np.uint32)
    ref = rng.integers(0, 6, size=n).astype(np.uint8)
    off = begin(bc, [(1, 0, n)], planes)
    check(bc, planes, off)
    check(bc, planes, off, iupac=True, call_ppm=200000, ref=ref)
    check(bc, planes, off, iupac=True, call_ppm=200001, ref=ref, fill_ref=True)
    check(bc, planes, off, min_count=cm.M32, min_depth=5 * cm.M32 - 4, ref=ref)
    check(bc, planes, off, min_count=cm.M32 - 1, call_ppm=1000000)


# ------------------------------------------------------------ the int32 edge

def test_int32_edge(bc, P):
    """The consensus of reads around 2^31 and with reference ends below 2^32
    (bases_model.int32_edge_case), counted by the pileup kernel, with the
    segments in two orders."""
    reads, segs, scrambled, k = bm.int32_edge_case(P)
    b = bm.make_batch(reads)
    for sg in (segs, scrambled):
        off = begin(bc, sg)
        bc.add_reads(*bm.batch_args(b))
        tids, starts, ends = (np.array(x, np.int64) for x in zip(*sg))
        want_off, planes = bm.counts_model(b, tids, starts, ends)
        assert np.array_equal(off, want_off) and np.array_equal(bc.counts(), planes)
        got = check(bc, planes, off)
        assert (got.summary[:, mb.CALLED] > 0).all()                       # every segment has called letters
        check(bc, planes, off, min_depth=2, iupac=True, call_ppm=200000)
        ref = np.random.default_rng(10).integers(0, 5, size=planes.shape[1]).astype(np.uint8)
        check(bc, planes, off, min_depth=3, fill_ref=True, ref=ref)


# ----------------------------------------------------------------- segments

def test_segment_shapes(bc, P):
    rng = np.random.default_rng(12)
    lens = [1, 0, 2, 3, 5, 4, P - 1, P, P + 1, 2 * P + 1]
    segs = [(0, 10, 10 + L) for L in lens]
    segs += [(0, 10, 15), (0, 10, 15), (0, 12, 20), (1, 5, 5), (2, 0, 3), (0, 0, 0)]   # duplicated, overlapping, empty
    n = sum(e - s for _, s, e in segs)
    planes = random_planes(rng, n)
    off = begin(bc, segs, planes)
    assert set((off[:-1] % 4).tolist()) == {0, 1, 2, 3}
    ref = rng.integers(0, 5, size=n).astype(np.uint8)
    got = check(bc, planes, off)
    assert got.first[1] == got.first[2] and got.summary[1].tolist() == [0] * 8
    check(bc, planes, off, iupac=True, min_count=2, ref=ref)
    check(bc, planes, off, min_depth=6, call_ppm=400000, fill_ref=True, ref=ref)
    order = rng.permutation(len(segs))
    shuffled = [segs[i] for i in order]
    planes = random_planes(rng, n)
    check(bc, planes, begin(bc, shuffled, planes), iupac=True, ref=ref)
    # no segments at all, and only empty ones
    got = check(bc, np.zeros((6, 0), np.uint32), begin(bc, []))
    assert got.n == 0 and got.first.tolist() == [0]
    got = check(bc, np.zeros((6, 0), np.uint32), begin(bc, [(0, 3, 3), (1, 0, 0)]), fill_ref=True,
                ref=np.zeros(0, np.uint8))
    assert got.first.tolist() == [0, 0, 0]


def test_deletion_patterns(bc, P):
    rng = np.random.default_rng(13)
    L0 = 2 * P + 10
    segs = [(0, 0, L0), (0, 0, 37), (1, 100, 120), (2, 0, P + 3), (3, 7, 8), (3, 8, 9)]
    off = bm.seg_offsets([s[1] for s in segs], [s[2] for s in segs])
    planes = rng.integers(1, 4, size=(6, int(off[-1]))).astype(np.uint32)
    planes[bm.DEL] = 0
    dele = np.zeros(int(off[-1]), bool)
    dele[P - 5:P + 6] = True                      # a run across the first tile edge (segment 0 starts at index 0)
    dele[2 * P - 1:2 * P + 1] = True              # and across the second
    dele[off[1]:off[2]] = True                    # an all-deleted segment
    dele[[off[2], off[3] - 1]] = True             # a segment's first and last position
    dele[off[3]:off[4]:2] = True                  # alternating deleted and kept
    dele[off[4]] = True                           # a one-position segment, deleted; its neighbour kept
    planes[bm.DEL, dele] = 9
    assert np.array_equal(begin(bc, segs, planes), off)
    got = check(bc, planes, off)
    assert got.first[1] == got.first[2] and len(got.compact(1)) == 0
    assert bytes(got.aligned(1)) == b"-" * 37
    a = got.aligned(2)
    assert a[0] == DASH and a[-1] == DASH and (a[1:-1] != DASH).all() and len(got.compact(2)) == 18
    a = got.aligned(3)
    assert (a[0::2] == DASH).all() and (a[1::2] != DASH).all()
    assert got.summary[3, mb.DELETED] == (P + 4) // 2 and got.summary[0, mb.DELETED] == 13
    assert got.summary[4].tolist() == [1, 0, 0, 0, 0, 1, 0, 0] and got.summary[5, mb.LENGTH] == 1
    ref = rng.integers(0, 5, size=planes.shape[1]).astype(np.uint8)
    got = check(bc, planes, off, ref=ref, iupac=True)
    assert got.summary[1, mb.DIFFERS] == int((ref[off[1]:off[2]] < 4).sum())
    # the deletions no longer qualify: every position is kept
    got = check(bc, planes, off, min_count=10)
    assert got.n == planes.shape[1] and got.summary[:, mb.DELETED].sum() == 0


def test_many_one_position_segments(bc):
    """5000 segments of one position each: more tiles than one scan iteration."""
    rng = np.random.default_rng(14)
    S = 5000
    segs = [(int(rng.integers(0, N_REF)), i, i + 1) for i in rng.integers(0, 10 ** 6, size=S).tolist()]
    planes = random_planes(rng, S, p_del=0.3)
    off = begin(bc, segs, planes)
    assert bc.timing()["tiles"] == S
    ref = rng.integers(0, 5, size=S).astype(np.uint8)
    got = check(bc, planes, off, ref=ref)
    assert 0 < got.n < S and got.summary[:, mb.POSITIONS].tolist() == [1] * S
    check(bc, planes, off, iupac=True, min_count=2)


# ---------------------------------------------------------------- reference

def test_reference_plane(bc, P):
    rng = np.random.default_rng(15)
    segs = [(0, 3, P + 40), (1, 0, 300)]
    n = sum(e - s for _, s, e in segs)
    planes = random_planes(rng, n, p_empty=0.3)
    ref = rng.integers(0, 256, size=n).astype(np.uint8)           # mostly unknown codes
    ref[::3] = rng.integers(0, 4, size=len(ref[::3]))
    off = begin(bc, segs, planes)
    plain = check(bc, planes, off)
    assert plain.summary[:, mb.DIFFERS].sum() == 0                # no reference: nothing differs
    got = check(bc, planes, off, ref=ref)
    assert 0 < got.summary[:, mb.DIFFERS].sum() < (ref < 4).sum()
    assert np.array_equal(got.summary[:, :mb.DIFFERS], plain.summary[:, :mb.DIFFERS])
    filled = check(bc, planes, off, ref=ref, fill_ref=True, min_depth=4)
    a = np.concatenate([filled.aligned(0), filled.aligned(1)])
    lower = np.isin(a, np.frombuffer(b"acgt", np.uint8))
    assert lower.any() and (ref[lower] < 4).all()
    assert np.array_equal(a[lower], np.frombuffer(b"acgt", np.uint8)[ref[lower]])
    assert filled.summary[:, mb.LOW].sum() > lower.sum()          # unknown codes stay N


# --------------------------------------------------------- state and errors

def _code(call):
    with pytest.raises(_lib.MetacovError) as e:
        call()
    return e.value.code


def _sites_now(h, n):
    """The current sites, fetched without computing them again."""
    first = np.zeros(h._S + 1, np.int64)
    _lib.check(h._lib.mc_bases_sites_first(h._h, _lib.ptr(first)), h._lib)
    pos, cnt = np.zeros(n, np.int64), np.zeros((n, 6), np.uint32)
    _lib.check(h._lib.mc_bases_sites_get(h._h, 0, n, _lib.ptr(pos), _lib.ptr(cnt)), h._lib)
    return first, pos, cnt


def test_state_and_errors(lib_built):
    lib = _lib.load()
    rng = np.random.default_rng(16)
    with mb.BaseCounter(2, 0) as h:
        out = np.zeros(64, np.int64)
        pa, pb = ctypes.c_void_p(), ctypes.c_void_p()
        raw = {"first": lambda: _lib.check(lib.mc_bases_consensus_first(h._h, _lib.ptr(out)), lib),
               "summary": lambda: _lib.check(lib.mc_bases_consensus_summary(h._h, _lib.ptr(out)), lib),
               "get": lambda: h.consensus_letters(False, 0, 1),
               "get_compact": lambda: h.consensus_letters(True, 0, 0),
               "device": lambda: _lib.check(lib.mc_bases_consensus_device(h._h, ctypes.byref(pa), ctypes.byref(pb)),
                                            lib)}
        # before begin
        for call in (lambda: h.consensus(), lambda: h.set_counts(0, np.zeros((6, 0), np.uint32)),
                     lambda: h.consensus_timing(), *raw.values()):
            assert _code(call) == _lib.MC_E_STATE
        n = h.begin([0, 1], [0, 10], [40, 30])
        assert n == 60
        for call in raw.values():                                  # begun, but no consensus yet
            assert _code(call) == _lib.MC_E_STATE
        planes = random_planes(rng, n, p_del=0.3)
        h.set_counts(0, planes)
        c = h.consensus()
        assert 0 < c.n < n
        for call in raw.values():
            call()
        assert pa.value and pb.value and pa.value != pb.value
        t = h.consensus_timing()
        assert t["call_ms"] > 0 and t["scan_ms"] > 0 and t["emit_ms"] > 0
        # every invalid argument; none of them drops the current consensus
        ref = np.zeros(n, np.uint8)
        for kw in (dict(min_depth=-1), dict(min_count=-1), dict(call_ppm=-1), dict(call_ppm=1000001),
                   dict(fill_ref=True)):
            assert _code(lambda: h.consensus(**kw)) == _lib.MC_E_INVALID, kw
            raw["get"]()
        tot = ctypes.c_int64()
        assert lib.mc_bases_consensus(h._h, 1, 1, 0, 4, _lib.ptr(ref), ctypes.byref(tot)) == _lib.MC_E_INVALID
        assert lib.mc_bases_consensus(h._h, 1, 1, 0, 0x80000001, None, ctypes.byref(tot)) == _lib.MC_E_INVALID
        one = np.zeros(8, np.uint8)
        for compact, first, count in ((0, -1, 1), (0, 0, -1), (0, n, 1), (0, n + 1, 0), (0, n - 1, 2), (0, 0, n + 1),
                                      (1, c.n, 1), (1, c.n + 1, 0), (1, 0, c.n + 1), (1, -1, 1)):
            rc = lib.mc_bases_consensus_get(h._h, compact, first, count, _lib.ptr(one))
            assert rc == _lib.MC_E_INVALID, (compact, first, count)
        assert lib.mc_bases_consensus_get(h._h, 0, n, 0, None) == 0          # the empty range at the end is fine
        assert lib.mc_bases_consensus_get(h._h, 1, c.n, 0, None) == 0
        for first, cnt in ((-1, 1), (n, 1), (n - 1, 2)):
            assert _code(lambda: h.set_counts(first, np.zeros((6, cnt), np.uint32))) == _lib.MC_E_INVALID
        assert np.array_equal(h.consensus_letters(False, 0, n), cm.call(planes)[0])
        # sites survive a consensus call, and a consensus survives a sites call
        s = h.sites(2, 1, 0)
        before = _sites_now(h, len(s))
        c = h.consensus(iupac=True, min_count=2)
        after = _sites_now(h, len(s))
        assert len(s) > 0 and all(np.array_equal(x, y) for x, y in zip(before, after))
        assert np.array_equal(after[1], s.pos) and np.array_equal(after[2], s.counts)
        want = cm.consensus_model(planes, h.seg_off, iupac=True, min_count=2)
        assert np.array_equal(c.aligned(1), want[2][40:])
        h.sites(1, 1, 0, ref=np.full(n, 2, np.uint8))
        assert np.array_equal(h.consensus_letters(False, 0, n), want[2])
        assert np.array_equal(h.consensus_letters(True, 0, c.n), want[3])
        first = np.zeros(3, np.int64)
        _lib.check(lib.mc_bases_consensus_first(h._h, _lib.ptr(first)), lib)
        assert np.array_equal(first, want[0])
        # add_reads and set_counts drop it (and the sites)
        h.add_reads(*bm.batch_args(bm.make_batch([(0, 1, "2M", "CG", 30)])))
        for call in raw.values():
            assert _code(call) == _lib.MC_E_STATE
        planes[bm.C, 1] += 1
        planes[bm.G, 2] += 1
        assert np.array_equal(h.counts(), planes)
        c = h.consensus()
        raw["get"]()
        h.set_counts(3, np.zeros((6, 2), np.uint32))
        for call in raw.values():
            assert _code(call) == _lib.MC_E_STATE
        assert _code(lambda: _sites_now(h, 0)) == _lib.MC_E_STATE
        planes[:, 3:5] = 0
        c = h.consensus()
        assert np.array_equal(c.aligned(0), cm.call(planes)[0][:40])
        # a second begin drops it as well
        h.begin([0], [0], [4])
        for call in raw.values():
            assert _code(call) == _lib.MC_E_STATE


# --------------------------------------------------------------- end to end

def random_cigar(rng, P):
    ops = []
    for _ in range(int(rng.integers(1, 7))):
        op = int(rng.choice([0, 0, 0, 0, 1, 2, 2, 2, 3, 4, 7, 8]))
        n = int(rng.integers(1, 300)) if rng.random() < 0.9 else int(rng.integers(P, P + 50))
        if op in (1, 4):
            n = int(rng.integers(1, 12))
        ops.append("%d%s" % (n, bm.OPS[op]))
    return "".join(ops)


@pytest.mark.parametrize("seed", range(20))
def test_fuzz_through_pileup(bc, P, seed):
    rng = np.random.default_rng(300 + seed)
    L = 2 * P + int(rng.integers(0, 50))
    reads = []
    for _ in range(int(rng.integers(30, 90))):
        c = random_cigar(rng, P)
        n = bm.query_length(bm.cigar_words(c))
        reads.append((int(rng.integers(0, 2)), int(rng.integers(0, L)), c,
                      rng.choice([1, 2, 4, 8, 15], size=n, p=[.3, .3, .18, .18, .04]).tolist(), 30))
    segs = []
    for _ in range(int(rng.integers(1, 6))):
        a = int(rng.integers(0, L))
        segs.append((int(rng.integers(0, 2)), a, a + int(rng.integers(0, L))))
    b = bm.make_batch(sorted(reads, key=lambda r: (r[0], r[1])))
    tids, starts, ends = (np.array(x, np.int64) for x in zip(*segs))
    bc.begin(tids, starts, ends)
    bc.add_reads(*bm.batch_args(b))
    off, planes = bm.counts_model(b, tids, starts, ends)
    assert np.array_equal(bc.counts(), planes)
    ref = rng.integers(0, 5, size=planes.shape[1]).astype(np.uint8) if seed % 2 else None
    check(bc, planes, off, min_depth=int(rng.integers(0, 4)), min_count=int(rng.integers(0, 3)),
          call_ppm=int(rng.integers(0, 700000)), iupac=bool(seed % 3 == 0), fill_ref=bool(seed % 4 == 1), ref=ref)


GOLDENS = {"bbmap.sorted.bam": "reference_1K.fa.gz", "synth_exp.bam": "synth_exp.fa"}
_cache = {}


def golden(golden_dir, name):
    """(path, fasta path, names, lengths, the kept reads as one batch,
    sequences), read once per file."""
    if name not in _cache:
        path = os.path.join(golden_dir, name)
        names, lengths, b, _ = bm.kept_reads(path)
        fa = os.path.join(golden_dir, GOLDENS[name])
        _cache[name] = (path, fa, [w.split()[0] for w in names], lengths, b, bm.read_fasta(fa))
    return _cache[name]


def region_planes(g, regs):
    """Model planes, reference codes and seg_off of regions (tid, start, end),
    computed once per set of regions.  A read that overhangs its contig
    counts where it lies; the reference has no base there."""
    path, _, names, lengths, b, seqs = g
    key = (path, tuple(regs))
    if key not in _cache:
        tids, starts, ends = (np.array(x, np.int64) for x in zip(*regs))
        seg_off, planes = bm.counts_model(b, tids, starts, ends)
        codes = [np.array([{"A": 0, "C": 1, "G": 2, "T": 3}.get(ch, 4)
                           for ch in (seqs.get(names[t], "").upper() + "N" * e)[a:e]], np.uint8) for t, a, e in regs]
        _cache[key] = (planes, np.concatenate(codes), seg_off)
    return _cache[key]


VARIANTS = {
    "compact": ([], dict(), False, False),
    "aligned_ref": (["--aligned", "-f", "FA"], dict(), True, False),
    "iupac_fill": (["--iupac", "--call-frac", "0.2", "--min-count", "2", "-f", "FA", "--fill-ref", "--min-depth", "3",
                    "--line-width", "0"],
                   dict(iupac=True, call_ppm=200000, min_count=2, fill_ref=True, min_depth=3), False, False),
    "regions_aligned": (["-rc", "RC", "--aligned", "--iupac", "-f", "FA", "--fill-ref", "--min-depth", "2",
                         "--line-width", "50"], dict(iupac=True, fill_ref=True, min_depth=2), True, True),
    "regions_compact": (["-rc", "RC", "--min-depth", "2"], dict(min_depth=2), False, True),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_cli(golden_dir, tmp_path, name, variant):
    from metacov_amd.cli import main
    g = golden(golden_dir, name)
    path, fa, names, lengths = g[:4]
    args, kw, aligned, with_regions = VARIANTS[variant]
    big = int(np.argmax(lengths))
    if with_regions:
        regs = [(big, 5, min(lengths[big], 700)), (0, 0, lengths[0]), (big, lengths[big] - 20, lengths[big] + 15),
                (big, 5, min(lengths[big], 700))]
        labels = ["%s:%d-%d" % (names[t], a + 1, b) for t, a, b in regs]
        rc = tmp_path / "r.csv"
        rc.write_text("sequence_id,start,stop\n" + "".join("%s,%d,%d\n" % (names[t], a, b) for t, a, b in regs))
    else:
        regs = [(t, 0, L) for t, L in enumerate(lengths)]
        labels = names
    planes, codes, seg_off = region_planes(g, regs)
    use_ref = "-f" in args
    first, summary, letters, compact = cm.consensus_model(planes, seg_off, ref=codes if use_ref else None, **kw)
    width = int(args[args.index("--line-width") + 1]) if "--line-width" in args else 60
    want = "".join(cm.fasta(labels[s], letters[seg_off[s]:seg_off[s + 1]] if aligned
                            else compact[first[s]:first[s + 1]], width) for s in range(len(regs)))
    want_summary = cm.summary_table([(names[t], a, b, summary[s]) for s, (t, a, b) in enumerate(regs)])
    args = [fa if a == "FA" else str(tmp_path / "r.csv") if a == "RC" else a for a in args]
    texts = []
    for decode in ("host", "gpu"):
        out, tsv = tmp_path / ("%s.fa" % decode), tmp_path / ("%s.tsv" % decode)
        r = CliRunner().invoke(main, ["consensus", "-b", path, "-o", str(out), "--summary", str(tsv), "--decode",
                                      decode] + args)
        assert r.exit_code == 0, r.output
        texts.append(out.read_bytes())
        assert tsv.read_text() == want_summary
    assert texts[0] == texts[1]
    assert texts[0].decode() == want
    assert summary[:, cm.COL_CALLED].sum() > 0


def test_consensus_convenience(golden_dir):
    g = golden(golden_dir, "bbmap.sorted.bam")
    path, fa, names, lengths, b, seqs = g
    t = int(np.argmax(lengths))
    p, codes, seg_off = region_planes(g, [(t, 0, lengths[t])])
    first, summary, letters, compact = cm.consensus_model(p, seg_off)
    got, row = mb.consensus(path, names[t])
    assert got.dtype == np.uint8 and np.array_equal(got, compact) and np.array_equal(row, summary[0])
    a, b = 10, lengths[t] // 2
    p, codes, seg_off = region_planes(g, [(t, a, b)])
    ref = (seqs.get(names[t], "") + "N" * b)[a:b]
    want = cm.consensus_model(p, seg_off, ref=codes, iupac=True, fill_ref=True, min_depth=3, call_ppm=250000)
    for decode in ("host", "gpu"):
        got, row = mb.consensus(path, names[t], a, b, min_depth=3, call_ppm=250000, iupac=True, fill_ref=True, ref=ref,
                                aligned=True, decode=decode)
        assert np.array_equal(got, want[2]) and np.array_equal(row, want[1][0])
    with pytest.raises(KeyError):
        mb.consensus(path, "no_such_contig")
    with pytest.raises(ValueError):
        mb.consensus(path, names[t], 0, 10, ref="ACGT")
