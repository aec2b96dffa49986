"""htslib's pileup read cap (pysam's max_depth, on by default): the library's closed form
(mc_depth_cap_mask, host C++) against a literal restatement of htslib's
bam_plp_push / bam_plp_next loop (oracle/htslib_plp.py), per region query
the way pysam's AlignmentFile.pileup(ref, start, end) runs it
(metacov/pileup.py:13).  Parity with htslib itself is unpinned (htslib is
absent here and the cap is version-dependent)."""
import functools
import os

import numpy as np
import pytest

from metacov_amd import depthcap
from oracle import htslib_plp


def kept_depth(pos, span, keep, start, end):
    """classic()'s column vector from the kept reads (difference array; a
    span-0 read adds nothing, as current htslib's bam_plp_push)."""
    d = np.zeros(end - start + 1, np.int64)
    for p, s in zip(pos[keep], span[keep]):
        a, b = max(p, start), min(p + s, end)
        if b > a:
            d[a - start] += 1
            d[b - start] -= 1
    return np.cumsum(d)[:-1]


def piles(rng, n_piles, pile_size, bg, L, span_rng):
    starts = [int(x) for x in rng.integers(0, L - 400, size=n_piles)]
    pos = [np.full(pile_size, s) for s in starts]
    pos.append(rng.integers(0, L - 200, size=bg))
    pos = np.concatenate(pos)
    span = rng.integers(span_rng[0], span_rng[1] + 1, size=len(pos))
    span = np.minimum(span, L - pos)
    o = np.argsort(pos, kind="stable")
    return pos[o].astype(np.int32), span[o].astype(np.int32)


@pytest.mark.parametrize("cap,n_piles,pile,bg,seed,smin", [
    (5, 20, 12, 300, 1, 1), (20, 10, 40, 500, 2, 1), (64, 6, 150, 2000, 3, 1), (3, 50, 6, 100, 4, 1),
    (1, 10, 5, 50, 5, 1), (5, 20, 12, 300, 6, 0), (20, 10, 40, 500, 7, 0), (3, 50, 6, 100, 8, 0),
    (2, 30, 9, 200, 9, 0)])
def test_cap_mask_matches_literal_htslib(cap, n_piles, pile, bg, seed, smin):
    """smin = 0: span-0 reads (no reference-consuming op) in the piles and the
    background, which enter the pool only as a start group's first read."""
    rng = np.random.default_rng(seed)
    L = 5000
    pos, span = piles(rng, n_piles, pile, bg, L, (smin, 300))
    if smin == 0:
        span[rng.random(len(span)) < 0.15] = 0
    tid = np.zeros(len(pos), np.int32)
    for (s, e) in [(0, L), (0, 1), (100, 2600), (2500, 4999), (1234, 1300)]:
        want, dropped = htslib_plp.region_depth(tid, pos, span, 0, s, e, max_depth=cap)
        idx = depthcap.region_reads(tid, pos, span, 0, s, e)
        keep, d2 = depthcap.cap_mask(tid[idx], pos[idx], span[idx], cap)
        assert d2 == dropped, (s, e)
        got = kept_depth(pos[idx], span[idx], keep, s, e)
        assert np.array_equal(got, want), (s, e)


def test_cap_8000_amplicon_piles():
    """Amplicon-like piles deeper than pysam's default cap: 3 starts with
    9000-12000 reads each over background coverage (> 8000x columns)."""
    rng = np.random.default_rng(11)
    L = 3000
    pos = np.concatenate([np.full(12_000, 500), np.full(9_000, 520), np.full(10_500, 1400),
                          rng.integers(0, 2800, size=4000)])
    span = np.concatenate([np.full(12_000, 150), rng.integers(100, 200, size=9_000),
                           np.full(10_500, 120), rng.integers(1, 200, size=4000)])
    o = np.argsort(pos, kind="stable")
    pos, span = pos[o].astype(np.int32), span[o].astype(np.int32)
    tid = np.zeros(len(pos), np.int32)
    want, dropped = htslib_plp.region_depth(tid, pos, span, 0, 0, L, max_depth=8000)
    keep, d2 = depthcap.cap_mask(tid, pos, span, 8000)
    assert dropped > 0 and d2 == dropped
    assert np.array_equal(kept_depth(pos, span, keep, 0, L), want)
    full = kept_depth(pos, span, np.ones(len(pos), bool), 0, L)
    assert full.max() > 8000 and want.max() < full.max()


def test_cap_mask_contigs_independent_and_errors():
    rng = np.random.default_rng(5)
    tid = np.repeat(np.arange(4, dtype=np.int32), 300)
    pos = np.concatenate([np.sort(rng.integers(0, 40, size=300)) for _ in range(4)]).astype(np.int32)
    span = rng.integers(1, 50, size=len(pos)).astype(np.int32)
    keep, _ = depthcap.cap_mask(tid, pos, span, 7, n_threads=3)
    for t in range(4):
        m = tid == t
        k1, _ = depthcap.cap_mask(tid[m], pos[m], span[m], 7, n_threads=1)
        assert np.array_equal(keep[m], k1)
    from metacov_amd._lib import MetacovError
    with pytest.raises(MetacovError):
        depthcap.cap_mask(np.zeros(2, np.int32), np.array([5, 3], np.int32), np.ones(2, np.int32), 7)
    with pytest.raises(MetacovError):
        depthcap.cap_mask(tid, pos, span, 0)


@pytest.mark.parametrize("seed", range(12))
def test_gate_never_misses_a_drop(seed):
    """depthcap.may_cap's bound: while 2 + 2 * (exact max depth of the region)
    <= max_depth, htslib's literal push/next loop drops nothing, so the
    exact row is the capped one.  Random piles sized around the bound, with
    span-0 reads and both end rules."""
    rng = np.random.default_rng(100 + seed)
    L = 600
    cap = int(rng.integers(4, 24))
    n = int(rng.integers(50, 400))
    pos = np.sort(np.concatenate([rng.integers(0, L - 50, size=n),
                                  np.full(int(rng.integers(0, cap)), int(rng.integers(0, L - 60)))]))
    span = rng.integers(0, 60, size=len(pos))
    span[rng.random(len(span)) < 0.2] = 0
    if seed % 2:
        span = np.maximum(span, 1)                      # legacy bam_endpos spans
    pos, span = pos.astype(np.int32), span.astype(np.int32)
    tid = np.zeros(len(pos), np.int32)
    checked = 0
    for _ in range(30):
        s = int(rng.integers(0, L - 1))
        e = int(rng.integers(s + 1, L + 20))
        exact = kept_depth(pos, span, np.ones(len(pos), bool), s, e)
        want, dropped = htslib_plp.region_depth(tid, pos, span, 0, s, e, max_depth=cap)
        if 2 + 2 * int(exact.max()) <= cap:
            checked += 1
            assert dropped == 0 and np.array_equal(want, exact), (s, e, cap)
        rows = np.zeros(1, dtype=[("max", np.int64)])
        rows["max"] = exact.max()
        assert depthcap.may_cap(rows, cap)[0] == (2 + 2 * int(exact.max()) > cap)


def test_zero_span_reads_and_the_pool():
    """A span-0 read that opens a start group occupies a pool node until its
    column, so a later read of the same group can be dropped because of it;
    one inside a group never joins the pool (bam_plp_push: tail->end > pos)."""
    pos = np.array([10, 10, 10, 10, 20, 20, 20], np.int32)
    span = np.array([0, 5, 5, 5, 5, 0, 5], np.int32)
    tid = np.zeros(len(pos), np.int32)
    for cap in (1, 2, 3, 4):
        want, dropped = htslib_plp.region_depth(tid, pos, span, 0, 0, 40, max_depth=cap)
        keep, d2 = depthcap.cap_mask(tid, pos, span, cap)
        assert d2 == dropped, cap
        assert np.array_equal(kept_depth(pos, span, keep, 0, 40), want), cap


# ---- the device walk (csrc/capmask.h) --------------------------------------

def _model_case(rng, cap, pile, bg, L, smin, inq_frac=0.0):
    pos, span = piles(rng, int(rng.integers(1, 12)), pile, bg, L, (smin, 300))
    if smin == 0:
        span[rng.random(len(span)) < 0.15] = 0
    inq = np.ones(len(pos), np.uint8)
    if inq_frac:
        inq[rng.random(len(pos)) < inq_frac] = 0
    return pos, span, inq


@pytest.mark.parametrize("seed", range(24))
def test_device_walk_model_matches_host_closed_form(seed):
    """tests/cap_model.py (cap_walk_kernel lane for lane: bulk chunks, groups
    in lane order, the ring of ends) against mc_depth_cap_mask on the reads
    of the query; reads outside the query are invisible to the walk and keep
    0; small rings take the wrap-around and gap paths."""
    from tests import cap_model
    rng = np.random.default_rng(100 + seed)
    cap = int(rng.choice([1, 2, 3, 5, 20, 64, 100, 300]))
    pile = int(rng.choice([3, 12, 40, 70, 150, 400]))
    pos, span, inq = _model_case(rng, cap, pile, int(rng.integers(0, 600)), 5000, int(rng.integers(0, 2)),
                                 inq_frac=0.2 if seed % 3 == 0 else 0.0)
    ring = int(rng.choice([512, 1024, 32768]))
    keep, out_span, dropped = cap_model.cap_walk(list(pos), list(span), list(inq), cap, int(span.max(initial=0)),
                                                 ring=ring)
    sel = np.nonzero(inq)[0]
    want, wd = depthcap.cap_mask(np.zeros(len(sel), np.int32), pos[sel], span[sel], cap)
    assert dropped == wd
    got = np.array(keep, bool)
    assert not got[inq == 0].any()
    assert np.array_equal(got[sel], want)
    assert np.array_equal(np.array(out_span), np.where(got, span, 0))


def test_device_walk_model_deep_pile():
    """A 20,000x pile at the 8000 cap: groups larger than a chunk, bulk
    stretches before and after."""
    from tests import cap_model
    rng = np.random.default_rng(9)
    pos = np.sort(np.concatenate([rng.integers(0, 3000, 600), rng.integers(1000, 1150, 20000)])).astype(np.int32)
    span = rng.integers(0, 200, len(pos)).astype(np.int32)
    keep, _, dropped = cap_model.cap_walk(list(pos), list(span), [1] * len(pos), 8000, 200)
    want, wd = depthcap.cap_mask(np.zeros(len(pos), np.int32), pos, span, 8000)
    assert dropped == wd > 0
    assert np.array_equal(np.array(keep, bool), want)


@pytest.mark.gpu
def test_device_cap_mask_matches_host(lib_built):
    """mc_depth_cap_mask_device against mc_depth_cap_mask and the literal
    htslib restatement: many queries (tids) in one call, span-0 reads,
    8000-cap amplicon piles, unsorted input refused."""
    import torch
    rng = np.random.default_rng(21)
    tids, poss, spans = [], [], []
    for t in range(40):
        cap_case = t % 4
        pos, span = piles(rng, int(rng.integers(1, 8)), [12, 60, 150, 2500][cap_case], int(rng.integers(0, 800)),
                          6000, (0 if t % 2 else 1, 300))
        if t % 2:
            span[rng.random(len(span)) < 0.15] = 0
        tids.append(np.full(len(pos), t, np.int32))
        poss.append(pos)
        spans.append(span)
    tid, pos, span = (np.concatenate(x) for x in (tids, poss, spans))
    for cap in (3, 40, 8000, 1):
        want, wd = depthcap.cap_mask(tid, pos, span, cap)
        got, gd = depthcap.cap_mask_device(*(torch.from_numpy(a).cuda() for a in (tid, pos, span)), cap)
        assert gd == wd
        assert np.array_equal(got.cpu().numpy().astype(bool), want)
    # one query against the literal pileup loop
    t0 = tid == 3
    idx = np.nonzero(t0)[0]
    got, gd = depthcap.cap_mask_device(*(torch.from_numpy(a[idx]).cuda() for a in (tid, pos, span)), 40)
    v, dropped = htslib_plp.region_depth(tid[idx], pos[idx], span[idx], 3, 0, 6000, max_depth=40)
    assert gd == dropped
    assert np.array_equal(kept_depth(pos[idx], span[idx], got.cpu().numpy().astype(bool), 0, 6000), v)
    bad = pos.copy()
    bad[5], bad[6] = bad[6] + 1, bad[5]
    with pytest.raises(Exception, match="sorted"):
        depthcap.cap_mask_device(*(torch.from_numpy(a).cuda() for a in (tid, bad, span)), 40)


@pytest.mark.gpu
def test_device_cap_mask_random_sets(lib_built):
    """Random query sets (1-30 contigs of random piles, background depth,
    span-0 share and cap from 1 to 9000): the device mask and drop count
    equal mc_depth_cap_mask's.  MC_CAP_SOAK_ITERS / MC_CAP_SOAK_SEED: soak
    runs (profiles/r06/r06soak_cap.txt)."""
    import torch
    rng = np.random.default_rng(int(os.environ.get("MC_CAP_SOAK_SEED", "77")))
    for _ in range(int(os.environ.get("MC_CAP_SOAK_ITERS", "4"))):
        tids, poss, spans = [], [], []
        for t in range(int(rng.integers(1, 31))):
            pos, span = piles(rng, int(rng.integers(1, 6)), int(rng.integers(5, 3000)), int(rng.integers(0, 400)),
                              int(rng.integers(800, 9000)), (int(rng.integers(0, 2)), int(rng.integers(2, 400))))
            span[rng.random(len(span)) < rng.random() * 0.3] = 0
            tids.append(np.full(len(pos), t, np.int32))
            poss.append(pos)
            spans.append(span)
        tid, pos, span = (np.concatenate(x) for x in (tids, poss, spans))
        cap = int(rng.choice([1, 2, 7, 50, 300, 2000, 8000, 9000]))
        want, wd = depthcap.cap_mask(tid, pos, span, cap)
        got, gd = depthcap.cap_mask_device(*(torch.from_numpy(a).cuda() for a in (tid, pos, span)), cap)
        assert gd == wd, cap
        assert np.array_equal(got.cpu().numpy().astype(bool), want), cap


@pytest.mark.gpu
def test_capped_rows_device_equals_host(lib_built, tmp_path):
    """capped_rows on a GPU decode (mc_add_reads_capped: gather, cap and
    batch in HBM) equals the host sweep on the same file's host decode, on
    8000-cap piles with span-0 reads, for regions that share a contig, start
    before / inside piles, run past the contig end, and on a contig shard."""
    from metacov_amd import synth
    from metacov_amd.bam import BamFile, GpuBamFile
    rng = np.random.default_rng(5)
    names, lengths, recs = ["a", "b", "c"], [6000, 3000, 9000], []
    for t, L in enumerate(lengths):
        pos, span = piles(rng, 3, [9000, 4100, 12000][t], 3000, L, (0, 300))
        span[rng.random(len(span)) < 0.05] = 0
        recs += [synth.SynthRecord("r%d_%d" % (t, i), t, int(p), 0, [(0, int(s))] if s else [(4, 20)], 0)
                 for i, (p, s) in enumerate(zip(pos, span))]
    bam = str(tmp_path / "deep.bam")
    synth.write_bam(bam, names, lengths, recs)
    regs = [(0, 0, 6000), (0, 1000, 2500), (2, 0, 9500), (1, 100, 2900), (2, 4000, 4100), (0, 5990, 6000)]
    t, s, e = (np.array([r[i] for r in regs], np.int64) for i in range(3))
    want, wd = depthcap.capped_rows(BamFile(bam), t, s, e, lengths)
    g = GpuBamFile(bam)
    got, gd = depthcap.capped_rows(g, t, s, e, lengths)
    assert gd == wd > 0
    assert np.array_equal(got, want)
    g.restrict([0, 2])
    sel = t != 1
    got2, gd2 = depthcap.capped_rows(g, t[sel], s[sel], e[sel], lengths)
    want2, wd2 = depthcap.capped_rows(BamFile(bam), t[sel], s[sel], e[sel], lengths)
    assert gd2 == wd2 and np.array_equal(got2, want2)
    g.close()


def _continuation_pile():
    """Start groups of 70 reads (longer than a 64-read chunk) whose tails are
    1 bp and span-0 reads, 3 positions apart, below the cap, then a pile
    at the cap: a bulk chunk must insert the open group's ends before it
    moves its pointer, or they linger and inflate the later pool count."""
    pos, span = [], []
    for s in range(0, 12000, 3):
        for j in range(70):
            pos.append(s)
            span.append((0 if j % 2 else 1) if j >= 60 else 1 + (j % 3))
    for j in range(400):
        pos.append(12100)
        span.append(50)
    return np.array(pos, np.int32), np.array(span, np.int32)


def test_device_walk_model_continuation_groups():
    from tests import cap_model
    pos, span = _continuation_pile()
    for cap in (120, 75, 300):
        keep, _, dropped = cap_model.cap_walk(list(pos), list(span), [1] * len(pos), cap, 3, ring=1024)
        want, wd = depthcap.cap_mask(np.zeros(len(pos), np.int32), pos, span, cap)
        assert dropped == wd and np.array_equal(np.array(keep, bool), want)


@pytest.mark.gpu
def test_device_cap_mask_continuation_groups(lib_built):
    import torch
    pos, span = _continuation_pile()
    tid = np.zeros(len(pos), np.int32)
    for cap in (120, 75, 300):
        want, wd = depthcap.cap_mask(tid, pos, span, cap)
        got, gd = depthcap.cap_mask_device(*(torch.from_numpy(a).cuda() for a in (tid, pos, span)), cap)
        assert gd == wd
        assert np.array_equal(got.cpu().numpy().astype(bool), want)


# ---- the device walk at real genome coordinates ----------------------------
# Positions beyond the ring: the ring of ends wraps, jumps reach and pass the
# ring size, spans reach the largest the device admits.

RING = 32768   # csrc/capmask.h: kCapRing (the LDS ring's slots); test_span_limit_of_the_device_walk pins it


def _device_mask(tid, pos, span, cap):
    import torch
    got, gd = depthcap.cap_mask_device(*(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (tid, pos, span)),
                                       cap)
    return got.cpu().numpy().astype(bool), gd


def _wraps(pos, span, keep):
    """Kept reads whose start and end lie in different turns of the ring."""
    p, s = pos.astype(np.int64)[keep], span.astype(np.int64)[keep]
    return int(np.count_nonzero(p // RING != (p + s) // RING))


@functools.lru_cache(maxsize=None)
def _translated_piles():
    """The short-span piles of the tests above (spans 0..300, 15 % span-0
    reads, positions below 6000), one copy per tid at each origin."""
    rng = np.random.default_rng(31)
    pos0, span0 = piles(rng, 7, 150, 900, 6000, (0, 300))
    span0[rng.random(len(span0)) < 0.15] = 0
    origins = [0, RING - 3000, 2 * RING - 100, 1_000_000_007, 2 ** 31 - 1 - 6400]
    pos = np.concatenate([pos0.astype(np.int64) + o for o in origins])
    assert (pos + np.tile(span0, len(origins))).max() < 2 ** 31
    tid = np.repeat(np.arange(len(origins), dtype=np.int32), len(pos0))
    return len(pos0), tid, pos.astype(np.int32), np.tile(span0, len(origins))


@pytest.mark.gpu
def test_device_cap_mask_translated_piles(lib_built):
    """Bulk path across the wrap: the same piles at origins 0, just below the
    ring size, just below twice it, 10^9 + 7 and just below 2^31, five tids in
    one call.  A mask must not depend on the origin."""
    n, tid, pos, span = _translated_piles()
    for cap in (3, 40, 8000):
        want, wd = depthcap.cap_mask(tid, pos, span, cap)
        assert _wraps(pos, span, want) > 0
        got, gd = _device_mask(tid, pos, span, cap)
        assert gd == wd and (cap == 8000 or wd > 0)
        assert np.array_equal(got, want)
        for k in range(1, len(tid) // n):
            assert np.array_equal(got[k * n:(k + 1) * n], got[:n]), (cap, k)


JUMP_GAPS = [8, 9, 300, 20000, RING - 65, RING - 64, RING - 1, RING, RING + 1, 100000, 3 * RING + 17, 5, 8, 9]
JUMP_GROUP = 40
JUMP_CAPS = (25, 60, 8000)


@functools.lru_cache(maxsize=None)
def _jump_groups():
    """15 start groups of 40 reads whose starts are JUMP_GAPS apart: every
    branch of CapWave::advance (a step of at most 8, a middle step, a step of
    at least the ring), spans from 0 to RING - 65 (the largest the device
    admits) around each gap, so live ends lie on both sides of the next start
    and of the ring's wrap.  Returns (origins, pos0 int64, span int32)."""
    rng = np.random.default_rng(32)
    starts = np.concatenate([[0], np.cumsum(JUMP_GAPS)])
    span = []
    for k in range(len(starts)):
        g = JUMP_GAPS[min(k, len(JUMP_GAPS) - 1)]
        span.append(rng.choice(np.clip([0, 1, g - 1, g, g + 1, RING - 65, 150], 0, RING - 65), size=JUMP_GROUP))
    pos0 = np.repeat(starts, JUMP_GROUP).astype(np.int64)
    span = np.concatenate(span).astype(np.int32)
    assert span.max() == RING - 65
    assert min(JUMP_GAPS) <= 8 and any(8 < g < RING for g in JUMP_GAPS) and max(JUMP_GAPS) >= RING
    top = int((pos0 + span).max())
    assert 400_000 < top < 440_000
    origins = (0, RING - 4, 1_000_000_007, 2 ** 31 - 1 - top)          # the last: the largest end is 2^31 - 1
    return origins, pos0, span


def _jump_case(origin):
    _, pos0, span = _jump_groups()
    pos = (pos0 + origin).astype(np.int32)
    assert int(pos[-1]) == int(pos0[-1]) + origin
    return np.zeros(len(pos), np.int32), pos, span


@functools.lru_cache(maxsize=None)
def _jump_host_masks():
    """mc_depth_cap_mask on the jump groups per (origin, cap), checked on the
    way: independent of the origin, reads dropped at the small caps, kept
    counts that differ from group to group, kept reads that wrap the ring."""
    origins = _jump_groups()[0]
    out = {}
    for cap in JUMP_CAPS:
        for o in origins:
            tid, pos, span = _jump_case(o)
            out[o, cap] = depthcap.cap_mask(tid, pos, span, cap)
            assert out[o, cap][1] == out[0, cap][1] and np.array_equal(out[o, cap][0], out[0, cap][0])
            assert _wraps(pos, span, out[o, cap][0]) > 0
        keep, dropped = out[0, cap]
        per_group = keep.reshape(-1, JUMP_GROUP).sum(axis=1)
        if cap == 8000:
            assert dropped == 0
        else:
            assert dropped > 0 and len(set(per_group.tolist())) > 2
    return out


@functools.lru_cache(maxsize=None)
def _jump_literal_depth():
    """The literal pileup loop at cap 60 on the jump groups at origin RING - 4,
    over [first start, last start + RING)."""
    tid, pos, span = _jump_case(RING - 4)
    s, e = int(pos[0]), int(pos[-1]) + RING
    return (s, e) + htslib_plp.region_depth(tid, pos, span, 0, s, e, max_depth=60)


def test_device_walk_model_jump_groups():
    """The jump groups on the CPU: the walk's model with the kernel's ring
    size against mc_depth_cap_mask at every origin and cap, and the host mask
    against the literal pileup loop (the device test uses the same input)."""
    from tests import cap_model
    origins = _jump_groups()[0]
    host = _jump_host_masks()
    for (o, cap), (want, wd) in host.items():
        tid, pos, span = _jump_case(o)
        keep, out_span, dropped = cap_model.cap_walk(pos.tolist(), span.tolist(), [1] * len(pos), cap,
                                                     int(span.max()), ring=RING)
        assert dropped == wd, (o, cap)
        assert np.array_equal(np.array(keep, bool), want), (o, cap)
        assert np.array_equal(np.array(out_span), np.where(want, span, 0))
    s, e, depth, dropped = _jump_literal_depth()
    tid, pos, span = _jump_case(origins[1])
    keep, wd = host[origins[1], 60]
    assert wd == dropped and np.array_equal(kept_depth(pos, span, keep, s, e), depth)


@pytest.mark.gpu
def test_device_cap_mask_jump_groups(lib_built):
    """Grouped path, all three advance branches, wrapped live ends: the
    device mask on the jump groups equals mc_depth_cap_mask's at every origin
    and cap, and at one origin the literal pileup loop's depth."""
    origins = _jump_groups()[0]
    host = _jump_host_masks()
    got = {}
    for (o, cap), (want, wd) in host.items():
        tid, pos, span = _jump_case(o)
        got[o, cap], gd = _device_mask(tid, pos, span, cap)
        assert gd == wd, (o, cap)
        assert np.array_equal(got[o, cap], want), (o, cap)
        assert np.array_equal(got[o, cap], got[0, cap]), (o, cap)
    s, e, depth, dropped = _jump_literal_depth()
    tid, pos, span = _jump_case(origins[1])
    assert host[origins[1], 60][1] == dropped
    assert np.array_equal(kept_depth(pos, span, got[origins[1], 60], s, e), depth)


HOLD_TRIPLES = [(15000, 20000), (RING - 100, 120), (20000, RING - 65), (9000, 30000), (300, 250)]


@functools.lru_cache(maxsize=None)
def _hold_queries():
    """The bulk path's hold condition (the ring must hold [ptr, last start +
    max span]): per query 30 reads at s, 30 at s + gap, both of span sp, and a
    pile of 300 at s + gap + 10, with a cap of 200.  The first chunk (the two
    groups and four reads of the pile) is far below the cap, so only the hold
    condition keeps it off the bulk path; gap + sp >= RING in the first four
    queries, so moving the pointer over the gap after inserting the second
    group's ends would clear them, and the pile would keep 30 reads too many.
    The last query fits the ring and is applied in bulk when it stands alone
    (max span 250).  Every query at four origins; returns (tid, pos, span)."""
    tid, pos, span = [], [], []
    for o in (0, RING - 4, 1_000_000_007, 2 ** 31 - 1 - 60_000):
        for gap, sp in HOLD_TRIPLES:
            assert (gap + sp >= RING) == (sp >= 20000 or gap >= 20000) and gap + 10 + sp < 60_000
            pos += [o] * 30 + [o + gap] * 30 + [o + gap + 10] * 300
            span += [sp] * 60 + [50] * 300
            tid += [len(tid) // 360] * 360
    return np.array(tid, np.int32), np.array(pos, np.int32), np.array(span, np.int32)


def _hold_expected(keep, dropped):
    """By hand: the pile's first read is kept, then reads while 1 + C + b <=
    200, C the live reads of the two groups (60, or 30 where the first
    group's reads end before the pile), b the pile's kept reads so far."""
    per = keep.reshape(-1, 360)
    assert per[:, :60].all()
    live = np.array([60 if sp > gap + 10 else 30 for gap, sp in HOLD_TRIPLES] * 4)
    assert np.array_equal(per[:, 60:].sum(axis=1), 200 - live) and dropped == int((100 + live).sum())
    assert all(row[60:60 + 200 - c].all() for row, c in zip(per, live))


def test_device_walk_model_bulk_hold():
    from tests import cap_model
    tid, pos, span = _hold_queries()
    want, wd = depthcap.cap_mask(tid, pos, span, 200)
    _hold_expected(want, wd)
    keep, dropped = np.zeros(len(tid), bool), 0
    for t in range(int(tid[-1]) + 1):
        m = tid == t
        k, _, d = cap_model.cap_walk(pos[m].tolist(), span[m].tolist(), [1] * 360, 200, int(span.max()), ring=RING)
        keep[m], dropped = np.array(k, bool), dropped + d
    assert dropped == wd and np.array_equal(keep, want)


@pytest.mark.gpu
def test_device_cap_mask_bulk_hold(lib_built):
    """The hold queries in one call (max span RING - 65: every query's first
    chunk is held), and the query that fits the ring alone (bulk)."""
    tid, pos, span = _hold_queries()
    want, wd = depthcap.cap_mask(tid, pos, span, 200)
    got, gd = _device_mask(tid, pos, span, 200)
    assert gd == wd and np.array_equal(got, want)
    _hold_expected(got, gd)
    m = np.isin(tid % len(HOLD_TRIPLES), [1, 4])                       # spans of at most 250
    assert span[m].max() == 250
    got, gd = _device_mask(tid[m], pos[m], span[m], 200)
    assert np.array_equal(got, want[m]) and gd == int((~want[m]).sum())


@pytest.mark.gpu
def test_span_limit_of_the_device_walk(lib_built):
    """Spans up to RING - 65 are walked on the device (the jump groups hold
    one); RING - 64 is refused with MC_E_RANGE, which capped_rows turns into
    the host sweep.  A change of kCapRing fails here."""
    from metacov_amd import _lib
    tid, pos, span = _jump_case(0)
    assert span.max() == RING - 65
    want, wd = depthcap.cap_mask(tid, pos, span, 60)
    got, gd = _device_mask(tid, pos, span, 60)
    assert gd == wd and np.array_equal(got, want)
    span = span.copy()
    span[int(np.argmax(span))] = RING - 64
    with pytest.raises(_lib.MetacovError) as e:
        _device_mask(tid, pos, span, 60)
    assert e.value.code == _lib.MC_E_RANGE


def _pile_bam(path, L, starts, seed, long_record=None):
    """One contig of L bp: a pile of 100 reads at each start with 40 reads
    around it, 300 reads anywhere, spans 0..300 with span-0 records (20S), and
    optionally one record (pos, skip) `10M <skip>N 10M`.  Returns the
    records' (tid, pos, span) in file order."""
    from metacov_amd import synth
    rng = np.random.default_rng(seed)
    pos = np.concatenate([np.full(100, s) for s in starts] +
                         [rng.integers(max(s - 300, 0), s + 300, size=40) for s in starts] +
                         [rng.integers(0, L - 400, size=300)])
    span = rng.integers(0, 301, size=len(pos))
    span[rng.random(len(span)) < 0.1] = 0
    o = np.argsort(pos, kind="stable")
    pos, span = pos[o], span[o]
    cigars = [[(0, int(s))] if s else [(4, 20)] for s in span]
    if long_record is not None:
        p, skip = long_record
        k = int(np.searchsorted(pos, p, "right"))
        pos, span = np.insert(pos, k, p), np.insert(span, k, skip + 20)
        cigars.insert(k, [(0, 10), (3, skip), (0, 10)])
    recs = [synth.SynthRecord("r%d" % i, 0, int(p), 0, c, 0) for i, (p, c) in enumerate(zip(pos, cigars))]
    synth.write_bam(path, ["c"], [L], recs)
    return np.zeros(len(pos), np.int32), pos.astype(np.int32), span.astype(np.int32)


def _capped_rows_both(bam, regs, L, cap, monkeypatch):
    """capped_rows of a GpuBamFile and of a BamFile (the host sweep) on the
    same file; the third value: whether the GpuBamFile call ran the host
    sweep (depthcap.cap_mask) itself."""
    from metacov_amd.bam import BamFile, GpuBamFile
    t, s, e = (np.array([r[i] for r in regs], np.int64) for i in range(3))
    want, wd = depthcap.capped_rows(BamFile(bam), t, s, e, [L], cap)
    calls = []
    host_mask = depthcap.cap_mask
    monkeypatch.setattr(depthcap, "cap_mask", lambda *a, **k: calls.append(1) or host_mask(*a, **k))
    g = GpuBamFile(bam)
    try:
        got, gd = depthcap.capped_rows(g, t, s, e, [L], cap)
    finally:
        g.close()
        monkeypatch.setattr(depthcap, "cap_mask", host_mask)
    assert gd == wd > 0
    assert np.array_equal(got, want)
    return got, bool(calls)


def _check_against_literal(rows, regs, which, iv, cap):
    from metacov_amd.engine import classic_stats
    from oracle.classic_np import classic_from_vector
    for k in which:
        t, s, e = regs[k]
        assert e - s <= 4000
        want, _ = htslib_plp.region_depth(*iv, t, s, e, max_depth=cap)
        assert want.max() > 0
        assert classic_stats(rows[k]) == classic_from_vector(want.astype(np.float64)), regs[k]


@pytest.mark.gpu
@pytest.mark.parametrize("long_record", [True, False])
def test_capped_rows_long_record_takes_the_host_sweep(lib_built, tmp_path, monkeypatch, long_record):
    """A 200 kbp contig with piles the cap cuts and one record spanning 45 kbp
    (a long N): the device refuses the span and capped_rows falls back to the
    host sweep; without that record the same file stays on the device.  Both
    equal the host decode's rows, and the literal pileup loop on small
    regions, one of them under the long record."""
    L, cap = 200_000, 60
    bam = str(tmp_path / "long.bam")
    iv = _pile_bam(bam, L, [5000, 5003, 70_000, 150_000], 41, (60_000, 45_000) if long_record else None)
    assert (iv[2].max() >= 40_000) == long_record and (long_record or iv[2].max() < RING - 64)
    regs = [(0, 0, L), (0, 4900, 5400), (0, 5003, 5100), (0, 69_900, 70_400), (0, 60_000, 105_020),
            (0, 149_000, L + 500)]
    rows, swept = _capped_rows_both(bam, regs, L, cap, monkeypatch)
    assert swept == long_record
    _check_against_literal(rows, regs, (1, 3), iv, cap)


@pytest.mark.gpu
def test_capped_rows_beyond_the_ring(lib_built, tmp_path, monkeypatch):
    """mc_add_reads_capped (gather, ranges and the inq walk) on a 1.5 Mbp
    contig with piles just below the ring size, at twice and past ten times
    it and at 1.2 Mbp: regions that start before, inside and after a pile,
    straddle a multiple of the ring, run past the contig end and share the
    contig."""
    L, cap = 1_500_000, 60
    bam = str(tmp_path / "far.bam")
    starts = [RING - 20, 2 * RING, 10 * RING + 7, 1_200_000]
    iv = _pile_bam(bam, L, starts, 42)
    regs = [(0, RING - 500, RING + 300),                 # starts before the pile, straddles the ring size
            (0, RING + 10, RING + 400),                  # starts inside the pile's reads
            (0, RING + 400, 2 * RING - 300),             # after it
            (0, 2 * RING - 1000, 2 * RING + 1000), (0, 2 * RING, 2 * RING + 1), (0, 2 * RING + 50, 3 * RING),
            (0, 10 * RING - 100, 10 * RING + 400), (0, 9 * RING + 5, 11 * RING + 5),
            (0, 1_199_000, L + 500), (0, 1_200_000, 1_200_100), (0, 0, 4 * RING)]
    rows, swept = _capped_rows_both(bam, regs, L, cap, monkeypatch)
    assert not swept
    _check_against_literal(rows, regs, (0, 6), iv, cap)
