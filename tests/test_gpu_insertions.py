"""Insertion alleles on the GPU (csrc/bases_ins.h: extract, scatter, sort,
encode and the consensus kernels) against the model in
tests/insertions_model.py.  Every comparison is exact: the table's rows and
segment offsets, and with MC_CONS_INS out_first, the summary, the inserted
columns and the compact letters.  P (tile positions) and the sort chunk come
from the library; shapes are a few tiles at most."""
import os

import numpy as np
import pytest
from click.testing import CliRunner

from metacov_amd import _lib
from metacov_amd import bases as mb
from tests import bases_model as bm
from tests import consensus_model as cm
from tests import insertions_model as im

pytestmark = pytest.mark.gpu

N_REF = 4
E = im.encode


@pytest.fixture(scope="module")
def bc(lib_built):
    h = mb.BaseCounter(N_REF, 0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def P(lib_built):
    return mb.dims()


@pytest.fixture(scope="module")
def CHUNK(lib_built):
    chunk, max_len = mb.ins_dims()
    assert max_len == im.MAX_LEN
    return chunk


def segments(segs):
    return tuple(np.array(x, np.int64) for x in zip(*segs)) if segs else (np.zeros(0, np.int64),) * 3


def count(bc, segs, batches):
    """begin with insertions, add the batches; returns seg_off."""
    bc.begin(*segments(segs), insertions=True)
    for b in ([batches] if isinstance(batches, dict) else batches):
        bc.add_reads(*bm.batch_args(b))
    return bc.seg_off


def got_bytes(ins):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in
                    (ins.first, ins.index, ins.length, ins.code, ins.other, ins.count))


def same(ins, t, seg_off):
    """An Insertions against a model table, array by array."""
    assert ins.index.dtype == np.int64 and ins.length.dtype == np.int32 and ins.code.dtype == np.uint64
    assert ins.other.dtype == np.uint8 and ins.count.dtype == np.uint32 and ins.first.dtype == np.int64
    assert len(ins) == len(t["i"]), "%d rows, the model has %d" % (len(ins), len(t["i"]))
    for name, a, b in (("index", ins.index, t["i"]), ("other", ins.other, t["other"]), ("len", ins.length, t["len"]),
                       ("code", ins.code, t["code"]), ("count", ins.count, t["count"])):
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, "%s differs first at row %d: got %s, want %s" % (name, bad[0], a[bad[0]], b[bad[0]])
    assert np.array_equal(ins.first, im.first_of(t, seg_off))
    assert got_bytes(ins) == im.table_bytes(t, seg_off)


def check_table(bc, t, seg_off, planes=None, thresholds=((0, 1, 0),)):
    for th in thresholds:
        want = t if th == (0, 1, 0) else im.filter_table(t, planes, *th)
        same(bc.insertions(*th), want, seg_off)


def check_cons(bc, planes, seg_off, t, **kw):
    """One consensus call with insertions against the model."""
    got = bc.consensus(insertions=True, **kw)
    first, summary, inserted, aligned, compact = im.consensus_model(planes, seg_off, t, **kw)
    S = len(seg_off) - 1
    assert got.inserted.dtype == np.int64 and got.inserted.shape == (S, 2)
    assert np.array_equal(got.first, first)
    bad = np.argwhere(got.summary != summary)
    assert len(bad) == 0, "summary differs first at (segment, column) %s" % (bad[0],)
    assert np.array_equal(got.inserted, inserted)
    assert got.n == len(compact) == int(first[-1])
    assert np.array_equal(bc.consensus_letters(False, 0, planes.shape[1]), aligned)       # unchanged
    got_compact = bc.consensus_letters(True, 0, got.n)
    bad = np.flatnonzero(got_compact != compact)
    assert len(bad) == 0, "compact differs first at %d: ...%s, want ...%s" % (
        bad[0], bytes(got_compact[max(bad[0] - 5, 0):bad[0] + 5]), bytes(compact[max(bad[0] - 5, 0):bad[0] + 5]))
    s = got.summary
    assert np.array_equal(s[:, mb.LENGTH], s[:, mb.POSITIONS] - s[:, mb.DELETED] + got.inserted[:, 1])
    assert np.array_equal(s[:, mb.LENGTH], np.diff(got.first))
    for i in range(min(S, 20)):
        assert np.array_equal(got.compact(i), compact[first[i]:first[i + 1]])
    return got


def uniform_batch(pos, allele_of_read, alleles, tid=0):
    """len(allele_of_read) reads `1M <len>I 1M` at (tid, pos), read r carrying
    alleles[allele_of_read[r]] (a string over ACGTN): built without a Python
    loop over the reads' bases.  The anchor is pos itself.  Returns (batch,
    its rows as (len, code, other, count) in table order)."""
    allele_of_read = np.asarray(allele_of_read, np.int64)
    n = len(allele_of_read)
    packed = [np.frombuffer(bm.pack_seq("A" + a + "C"), np.uint8) for a in alleles]
    lens = np.array([len(a) for a in alleles], np.int64)
    nbytes = np.array([len(p) for p in packed], np.int64)
    seq_off = np.concatenate([[0], np.cumsum(nbytes[allele_of_read])])
    seq = np.concatenate([packed[k] for k in allele_of_read.tolist()])
    l_seq = (lens[allele_of_read] + 2).astype(np.int32)
    cigar = np.empty((n, 3), np.uint32)
    cigar[:, 0] = cigar[:, 2] = (1 << 4) | 0
    cigar[:, 1] = (lens[allele_of_read] << 4) | 1
    qual_off = np.concatenate([[0], np.cumsum(l_seq.astype(np.int64))])
    b = {"tid": np.full(n, tid, np.int32), "pos": np.full(n, pos, np.int32), "l_seq": l_seq,
         "cig_off": np.arange(n + 1, dtype=np.int64) * 3, "cigar": cigar.reshape(-1),
         "seq_off": seq_off.astype(np.int64), "seq": seq, "qual_off": qual_off.astype(np.int64),
         "qual": np.full(int(qual_off[-1]), 30, np.uint8)}
    per = np.bincount(allele_of_read, minlength=len(alleles))
    rows, n_other = {}, 0
    for a, c in zip(alleles, per.tolist()):
        if c == 0:
            continue
        if len(a) > im.MAX_LEN or set(a) - set("ACGT"):
            n_other += c
        else:
            rows[(len(a), E(a))] = rows.get((len(a), E(a)), 0) + c
    out = [(k[0], k[1], 0, c) for k, c in sorted(rows.items())]
    if n_other:
        out.append((0, 0, 1, n_other))
    return b, out


# ------------------------------------------------- hand cases, batch splits

def test_hand_cases(bc):
    for reads, want in im.HAND:
        b = bm.make_batch(sorted(reads, key=lambda r: (r[0], r[1])))
        off = count(bc, im.SEG, b)
        same(bc.insertions(0, 1, 0), im.make_table(want), off)
        _, planes = bm.counts_model(b, [0], [100], [200])
        assert np.array_equal(bc.counts(), planes)                     # the planes beside them are the usual ones
    # all of them at once, with min_baseq: qualities never touch insertions
    reads = sorted((r for case, _ in im.HAND for r in case), key=lambda r: (r[0], r[1]))
    b = bm.make_batch(reads, seq_gap=1)
    bc.begin([0], [100], [200], min_baseq=31, insertions=True)
    bc.add_reads(*bm.batch_args(b))
    t = im.table_model(b, [0], [100], [200])
    assert len(t["i"]) > 15
    same(bc.insertions(0, 1, 0), t, bc.seg_off)


def test_segments_by_hand(bc):
    reads = [(0, 150, "2M2I2M", "AACGAA", 30)]
    segs = [(0, 100, 200), (0, 151, 152), (0, 100, 200), (0, 152, 160), (1, 100, 200), (0, 140, 152), (0, 0, 0)]
    b = bm.make_batch(reads)
    off = count(bc, segs, b)
    ins = bc.insertions(0, 1, 0)
    assert ins.index.tolist() == [51, 100, 152, 320] and ins.first.tolist() == [0, 1, 2, 3, 3, 3, 4, 4]
    assert [ins.sequence(k) for k in range(4)] == ["CG"] * 4
    same(ins, im.table_model(b, *segments(segs)), off)


def piles(rng, n, L, P):
    """Sorted reads in piles: many share a start, a third carry insertions."""
    starts = rng.integers(0, L, size=12)
    reads = []
    for _ in range(n):
        pos = int(rng.choice(starts))
        if rng.random() < 0.35:
            k = int(rng.choice([5, 9]))
            ins = "".join(rng.choice(list("AC"), int(rng.choice([1, 1, 2, 3]))).tolist())
            if rng.random() < 0.1:
                ins = "N"
            reads.append((0, pos, "%dM%dI%dM" % (k, len(ins), 5), "G" * k + ins + "T" * 5, 30))
        else:
            k = int(rng.integers(1, 60))
            reads.append((0, pos, "%dM" % k, "A" * k, 30))
    return sorted(reads, key=lambda r: (r[0], r[1]))


def test_one_batch_against_three(bc, P):
    rng = np.random.default_rng(41)
    L = P + 300
    reads = piles(rng, 400, L, P)
    b = bm.make_batch(reads)
    segs = [(0, 0, L + 50), (0, P - 20, P + 20)]
    t = im.table_model(b, *segments(segs))
    assert (t["count"] > 2).any() and t["other"].any()
    off = count(bc, segs, b)
    one = bc.insertions(0, 1, 0)
    same(one, t, off)
    # cut inside a pile: the reads on both sides of each cut share (tid, pos)
    pos = b["pos"]
    cuts = [c for c in range(1, len(pos)) if pos[c] == pos[c - 1]]
    c1, c2 = cuts[len(cuts) // 3], cuts[2 * len(cuts) // 3]
    parts = [bm.slice_batch(b, 0, c1), bm.slice_batch(b, c1, c2), bm.slice_batch(b, c2, len(pos))]
    count(bc, segs, parts)
    three = bc.insertions(0, 1, 0)
    assert got_bytes(three) == got_bytes(one) == im.table_bytes(t, off)
    assert bc.insertions_timing()["events"] == int(t["count"].sum())


@pytest.mark.parametrize("name", ["synth_exp.bam", "synth_edge.bam"])
def test_add_device_matches_add_reads(bc, golden_dir, name):
    path = os.path.join(golden_dir, name)
    names, lengths, b, _ = bm.kept_reads(path)
    segs = [(t, 0, L) for t, L in enumerate(lengths)]
    t = im.table_model(b, *segments(segs))
    assert len(t["i"]) > 10
    out = []
    with mb.BaseCounter(len(lengths), 0) as h:
        for decode in ("host", "gpu"):
            h.begin(*segments(segs), insertions=True)
            h.add_bam(path, decode=decode, max_reads=500)              # several batches
            ins = h.insertions(0, 1, 0)
            same(ins, t, h.seg_off)
            out.append(got_bytes(ins))
    assert out[0] == out[1]


# --------------------------------------------------------------- tile edges

def test_anchors_at_tile_edges(bc, P):
    # an anchor on the last position of a tile, the next M in the next tile; contigs (segments from 0) of
    # P - 1, P, P + 1 and 2P + 1 positions with an anchor on their last position, through a trailing I and
    # through an I whose next M lies past the segment
    lens = [P - 1, P, P + 1, 2 * P + 1]
    segs = [(t, 0, L) for t, L in enumerate(lens)]
    reads = []
    for t, L in enumerate(lens):
        reads.append((t, L - 3, "3M2I", "AAACG", 30))                  # trailing I: anchor L - 1
        reads.append((t, L - 2, "2M1I4M", "AATAAAA", 30))              # anchor L - 1, the M runs past the end
        reads.append((t, L - 1, "2M1I1M", "AAGA", 30))                 # anchor L: outside
        reads.append((t, 0, "1M3I1M", "ACCCA", 30))                    # anchor 0
        if L > P:
            reads.append((t, P - 3, "3M2I4M", "AAAGTAAAA", 30))        # anchor P - 1, next M in the next tile
            reads.append((t, P - 2, "3M1I1M", "AAATA", 30))            # anchor P: the next tile's first position
    reads.sort(key=lambda r: (r[0], r[1]))
    b = bm.make_batch(reads)
    t = im.table_model(b, *segments(segs))
    off = count(bc, segs, b)
    same(bc.insertions(0, 1, 0), t, off)
    for s, L in enumerate(lens):
        assert int(off[s]) + L - 1 in t["i"].tolist() and int(off[s]) in t["i"].tolist()
    # segments that start inside the contig: unaligned plane offsets (tiles shorter by their lead)
    segs = [(0, 5, 6), (3, 1, 2 * P + 1), (3, P - 1, P + 1), (2, 7, P + 1)]
    same_off = count(bc, segs, b)
    assert set((same_off[:-1] % 4).tolist()) != {0}
    same(bc.insertions(0, 1, 0), im.table_model(b, *segments(segs)), same_off)


def test_long_read_three_tiles(bc, P):
    """A read of span 3P + 5 with insertions in three tiles, beside short reads
    (the tile search window is as wide as the long read)."""
    k = 3 * P + 5
    a, c = P // 2, P + P // 3
    cig = "%dM2I%dM1I%dM33I%dM" % (a, c - a, 2 * P + 7 - c, k - (2 * P + 7))
    seq = "A" * a + "CG" + "A" * (c - a) + "T" + "A" * (2 * P + 7 - c) + "G" * 33 + "A" * (k - (2 * P + 7))
    reads = [(0, 10, cig, seq, 30)]
    reads += [(0, p, "2M1I2M", "AACAA", 30) for p in (10, P, 2 * P + 14, 3 * P + 1, 3 * P + 14)]
    reads.sort(key=lambda r: (r[0], r[1]))
    b = bm.make_batch(reads)
    segs = [(0, 0, 4 * P), (0, 2 * P, 3 * P)]
    t = im.table_model(b, *segments(segs))
    assert {11, 9 + a, 9 + c, 2 * P + 16} <= set(t["i"].tolist()) and t["other"].sum() == 2
    off = count(bc, segs, b)
    same(bc.insertions(0, 1, 0), t, off)
    # the same reads one per batch: the long read's window no longer covers the others' batches
    count(bc, segs, [bm.slice_batch(b, i, i + 1) for i in range(len(reads))])
    same(bc.insertions(0, 1, 0), t, off)


def test_int32_edge(bc, P):
    """Anchors at 2^31 - 2, 2^31 - 1, 2^31, on both sides of a tile edge below
    2^31 and below 2^32 behind a skip of 1.9 * 10^9 positions
    (bases_model.int32_edge_case): the table, its filters and the consensus
    with insertions, with the segments in two orders, the reads in one batch
    and in two."""
    H = 1 << 31
    reads, segs, scrambled, k = bm.int32_edge_case(P)
    b = bm.make_batch(reads)
    parts = [bm.slice_batch(b, 0, k), bm.slice_batch(b, k, bm.n_reads(b))]
    for sg in (segs, scrambled):
        tids, starts, ends = segments(sg)
        t = im.table_model(b, tids, starts, ends)
        off = count(bc, sg, b)
        one = bc.insertions(0, 1, 0)
        same(one, t, off)
        a, far = sg.index(segs[0]), sg.index(segs[1])
        for p in (H - 2, H - 1, H, segs[0][1] + P - 1, segs[0][1] + P):
            assert int(off[a]) + p - segs[0][1] in one.index.tolist(), p
        assert ((one.index >= off[far]) & (one.index < off[far + 1])).sum() == 1
        _, planes = bm.counts_model(b, tids, starts, ends)
        assert np.array_equal(bc.counts(), planes)
        check_table(bc, t, off, planes, [(0, 1, 0), (3, 2, 0), (1, 1, 300000)])
        got = check_cons(bc, planes, off, t)
        assert got.inserted[a, 0] >= 7 and got.inserted[far, 0] == 1
        check_cons(bc, planes, off, t, min_depth=2, min_count=2, call_ppm=200000, iupac=True)
        count(bc, sg, parts)
        assert got_bytes(bc.insertions(0, 1, 0)) == got_bytes(one)
        assert np.array_equal(bc.counts(), planes)


# --------------------------------------------------------------- sort sizes

def anchor_table(pos_index, rows):
    return im.make_table((pos_index, n, code, other, c) for n, code, other, c in rows)


def test_bucket_of_one_and_of_one_chunk(bc, P, CHUNK):
    rng = np.random.default_rng(42)
    b, rows = uniform_batch(7, [0], ["GAT"])
    off = count(bc, [(0, 0, 30)], b)
    same(bc.insertions(0, 1, 0), anchor_table(7, rows), off)
    # exactly CHUNK events in one tile, on two anchors, 9 alleles with an OTHER among them
    alleles = ["A", "C", "AA", "AC", "CA", "T" * 32, "G" * 33, "ANA", "ACGTACGT"]
    b1, rows1 = uniform_batch(100, rng.integers(0, len(alleles), size=CHUNK - 1000), alleles)
    b2, rows2 = uniform_batch(101, rng.integers(0, len(alleles), size=1000), alleles)
    off = count(bc, [(0, 0, P)], [b1, b2])
    assert bc.insertions_timing()["events"] == CHUNK
    t = im.make_table([(100, n, c, o, k) for n, c, o, k in rows1] + [(101, n, c, o, k) for n, c, o, k in rows2])
    same(bc.insertions(0, 1, 0), t, off)
    same(bc.insertions(0, 200, 0), im.make_table([r for r in im.table_rows(t) if r[4] >= 200]), off)


def test_bucket_of_two_chunks_and_one(bc, P, CHUNK):
    """2 * CHUNK + 1 events on one anchor with 50 distinct alleles: the network
    over global memory."""
    rng = np.random.default_rng(43)
    alleles = sorted({"".join(rng.choice(list("ACGT"), int(rng.integers(1, 12))).tolist()) for _ in range(80)})[:48]
    alleles += ["ACNT", "A" * 40]                                      # two ways to be OTHER: one row
    assert len(alleles) == 50
    which = np.concatenate([np.arange(50), rng.integers(0, 50, size=2 * CHUNK + 1 - 50)])
    b, rows = uniform_batch(P + 9, rng.permutation(which), alleles)
    assert len(rows) == 49 and sum(r[3] for r in rows) == 2 * CHUNK + 1
    off = count(bc, [(0, 0, 2 * P)], b)
    same(bc.insertions(0, 1, 0), anchor_table(P + 9, rows), off)


def test_70000_events_on_one_anchor(bc, P):
    rng = np.random.default_rng(44)
    b, rows = uniform_batch(3, rng.choice(3, size=70000, p=[0.5, 0.3, 0.2]), ["TT", "G", "TA"])
    off = count(bc, [(0, 0, 50)], b)
    assert len(rows) == 3 and sum(r[3] for r in rows) == 70000
    t = anchor_table(3, rows)
    same(bc.insertions(0, 1, 0), t, off)
    # depth at the anchor is 70000 (the M in front of the I)
    planes = bc.counts()
    assert int(im.depth_of(planes)[3]) == 70000
    check_table(bc, t, off, planes, [(70000, 1, 0), (70001, 1, 0), (1, int(rows[1][3]), 0), (1, 1, 300000)])
    got = check_cons(bc, planes, off, t)
    assert got.inserted.tolist() == [[1, 2]] and bytes(got.compact(0))[3:7] == b"ATTC"


# --------------------------------------------------- zero events, handle state

def _code(call):
    with pytest.raises(_lib.MetacovError) as e:
        call()
    return e.value.code


def test_no_insertions_at_all(bc, P):
    b = bm.make_batch([(0, 5, "10M2D3M", "A" * 13, 30), (1, 0, "2S5M", "A" * 7, 30), (1, 3, "3I5M", "C" * 8, 30)])
    off = count(bc, [(0, 0, 2 * P), (1, 0, 10), (2, 0, 0)], b)
    ins = bc.insertions(0, 1, 0)
    assert len(ins) == 0 and ins.first.tolist() == [0, 0, 0, 0]
    assert bc.insertions_timing()["events"] == 0
    _, planes = bm.counts_model(b, [0, 1, 2], [0, 0, 0], [2 * P, 10, 0])
    check_cons(bc, planes, off, im.make_table([]))
    # no segments at all
    bc.begin([], [], [], insertions=True)
    ins = bc.insertions()
    assert len(ins) == 0 and ins.first.tolist() == [0]
    assert bc.consensus(insertions=True).n == 0


def test_fresh_handle_with_nothing_to_hold(lib_built):
    """A handle whose buffers were never allocated: no tiles, no events, no
    rows that qualify."""
    with mb.BaseCounter(1, 0) as h:
        h.begin([], [], [], insertions=True)
        assert len(h.insertions()) == 0 and h.consensus(insertions=True).n == 0
        h.set_insertions([], [], [], [], [])
        assert len(h.insertions()) == 0
    b = bm.make_batch([(0, 5, "10M", "A" * 10, 30), (0, 6, "3M1I3M", "AAACAAA", 30)])
    with mb.BaseCounter(1, 0) as h:
        h.begin([0], [0], [30], insertions=True)
        h.add_reads(*bm.batch_args(b))
        _, planes = bm.counts_model(b, [0], [0], [30])
        t = im.table_model(b, [0], [0], [30])
        got = check_cons(h, planes, h.seg_off, t, min_count=2)         # no row qualifies: none is called
        assert got.inserted.tolist() == [[0, 0]] and len(h.insertions(1, 2, 0)) == 0
        got = check_cons(h, planes, h.seg_off, t)
        assert got.inserted.tolist() == [[1, 1]]


def test_state_and_errors(lib_built):
    lib = _lib.load()
    b = bm.make_batch([(0, 5, "3M2I3M", "AAACGAAA", 30)])
    out = np.zeros(64, np.int64)
    with mb.BaseCounter(2, 0) as h:
        raw = {"insertions": lambda: h.insertions(),
               "first": lambda: _lib.check(lib.mc_bases_insertions_first(h._h, _lib.ptr(out)), lib),
               "get": lambda: _lib.check(lib.mc_bases_insertions_get(h._h, 0, 0, None, None, None, None, None), lib),
               "timing": lambda: h.insertions_timing(),
               "set": lambda: h.set_insertions([], [], [], [], []),
               "cons_ins": lambda: _lib.check(lib.mc_bases_consensus_ins(h._h, _lib.ptr(out)), lib)}
        for call in raw.values():                                      # before begin
            assert _code(call) == _lib.MC_E_STATE
        assert lib.mc_bases_track_insertions(None, 1) == _lib.MC_E_INVALID
        assert lib.mc_bases_track_insertions(h._h, 2) == _lib.MC_E_INVALID
        # a handle that is not tracking: MC_E_STATE, and the flag is the unknown bit it always was
        h.begin([0], [0], [40])
        h.add_reads(*bm.batch_args(b))
        for call in raw.values():
            assert _code(call) == _lib.MC_E_STATE
        assert _code(lambda: h.consensus(insertions=True)) == _lib.MC_E_INVALID
        plain = h.consensus()
        assert plain.inserted is None
        # tracking: no table yet, then one
        h.begin([0], [0], [40], insertions=True)
        for k in ("first", "get", "cons_ins"):
            assert _code(raw[k]) == _lib.MC_E_STATE
        h.add_reads(*bm.batch_args(b))
        ins = h.insertions()
        assert im.table_rows(im.make_table(zip(ins.index, ins.length, ins.code, ins.other, ins.count))) == \
            [(7, 2, E("CG"), 0, 1)]
        raw["first"](), raw["get"]()
        assert h.insertions_timing()["extract_ms"] > 0 and h.insertions_timing()["group_ms"] > 0
        for th in ((-1, 1, 0), (1, -1, 0), (1, 1, -1), (1, 1, 1000001)):
            assert _code(lambda: h.insertions(*th)) == _lib.MC_E_INVALID
        one = np.zeros(4, np.int64)
        for first, cnt in ((-1, 1), (0, -1), (1, 1), (2, 0), (0, 2)):
            rc = lib.mc_bases_insertions_get(h._h, first, cnt, _lib.ptr(one), _lib.ptr(one), _lib.ptr(one),
                                             _lib.ptr(one), _lib.ptr(one))
            assert rc == _lib.MC_E_INVALID, (first, cnt)
        assert lib.mc_bases_insertions_get(h._h, 0, 1, None, None, None, None, None) == _lib.MC_E_INVALID
        # consensus without the flag leaves no inserted columns; with it they are there
        assert _code(raw["cons_ins"]) == _lib.MC_E_STATE
        h.consensus()
        assert _code(raw["cons_ins"]) == _lib.MC_E_STATE
        c = h.consensus(insertions=True)
        assert c.inserted.tolist() == [[1, 2]] and bytes(c.compact(0))[5:11] == b"AAACGA"
        # add_reads drops the table; a second begin clears the events
        h.add_reads(*bm.batch_args(b))
        assert _code(raw["first"]) == _lib.MC_E_STATE and _code(raw["cons_ins"]) == _lib.MC_E_STATE
        assert h.insertions().count.tolist() == [2]
        h.begin([0], [0], [40], insertions=True)
        assert len(h.insertions()) == 0 and h.insertions_timing()["events"] == 0
        h.add_reads(*bm.batch_args(b))
        assert h.insertions().count.tolist() == [1]
        # the hook: validation, and no reads behind it
        ok = ([3, 3, 3, 9], [1, 2, 0, 32], [3, 0, 0, 2 ** 64 - 1], [0, 0, 1, 0], [1, 2, 3, 2 ** 32 - 1])
        h.set_insertions(*ok)
        got = h.insertions(0, 1, 0)
        assert got.index.tolist() == ok[0] and got.count.tolist() == ok[4] and got.code.tolist() == ok[2]
        assert _code(lambda: h.add_reads(*bm.batch_args(b))) == _lib.MC_E_STATE
        bad = [([40], [1], [0], [0], [1]), ([-1], [1], [0], [0], [1]),           # outside [0, N)
               ([3, 2], [1, 1], [0, 0], [0, 0], [1, 1]),                         # not sorted
               ([3, 3], [1, 1], [0, 0], [0, 0], [1, 1]),                         # not unique
               ([3, 3], [0, 1], [0, 0], [1, 0], [1, 1]),                         # OTHER in front of an allele
               ([3, 3], [2, 1], [0, 0], [0, 0], [1, 1]),                         # longer in front of shorter
               ([3], [0], [0], [0], [1]), ([3], [33], [0], [0], [1]),            # len out of range
               ([3], [1], [4], [0], [1]), ([3], [1], [0], [1], [1]),             # code >= 4^len; OTHER with a len
               ([3], [1], [0], [2], [1]), ([3], [1], [0], [0], [0])]             # other not 0 / 1; count 0
        for rows in bad:
            assert _code(lambda: h.set_insertions(*rows)) == _lib.MC_E_INVALID, rows
        h.begin([0], [0], [40], insertions=True)                       # begin ends the hook's reign
        h.add_reads(*bm.batch_args(b))
        assert h.insertions().count.tolist() == [1]


# ------------------------------------- consensus through the two test hooks

def install(bc, segs, planes, rows):
    bc.begin(*segments(segs), insertions=True)
    bc.set_counts(0, planes)
    t = im.make_table(rows)
    bc.set_insertions(t["i"], t["len"], t["code"], t["other"], t["count"])
    same(bc.insertions(0, 1, 0), t, bc.seg_off)
    return bc.seg_off, t


def random_planes(rng, n, p_del=0.2, p_empty=0.1):
    planes = rng.integers(0, 4, size=(6, n)).astype(np.uint32)
    planes[bm.DEL] = np.where(rng.random(n) < p_del, rng.integers(3, 9, size=n), rng.integers(0, 2, size=n))
    planes[:, rng.random(n) < p_empty] = 0
    return planes


def random_rows(rng, index, max_alleles=3):
    """Sorted unique rows on the given plane indices."""
    rows = []
    for i in sorted(set(int(x) for x in index)):
        keys = set()
        for _ in range(int(rng.integers(1, max_alleles + 1))):
            n = int(rng.choice([1, 1, 2, 3, 7, 32]))
            keys.add((0, n, int(rng.integers(0, min(4 ** n, 2 ** 63)))))
        if rng.random() < 0.3:
            keys.add((1, 0, 0))
        rows += [(i, n, code, o, int(rng.integers(1, 5))) for o, n, code in sorted(keys)]
    return rows


def test_consensus_rule_by_hand(bc):
    A5, C5, D5, LOW = (5, 0, 0, 0, 0, 0), (0, 5, 0, 0, 0, 0), (0, 0, 0, 0, 0, 5), (0, 0, 0, 0, 3, 0)
    cases = [
        ([A5, C5, A5], [(1, 2, E("GT"), 0, 3), (1, 0, 0, 1, 9)], {}, "ACGTA"),
        ([A5, C5, A5], [(1, 0, 0, 1, 9)], {}, "ACA"),
        ([A5], [(0, 1, E("T"), 0, 2), (0, 2, E("AA"), 0, 2)], {}, "AT"),
        ([A5], [(0, 2, E("AC"), 0, 2), (0, 2, E("CA"), 0, 2)], {}, "AAC"),
        ([A5], [(0, 1, E("T"), 0, 2), (0, 2, E("AA"), 0, 2), (0, 3, E("GGG"), 0, 3)], {}, "AGGG"),
        ([A5, LOW, A5], [(1, 1, E("G"), 0, 4)], {}, "ANA"),
        ([A5, C5, A5], [(1, 1, E("G"), 0, 4)], dict(min_depth=6), "NNN"),
        ([A5, D5, C5], [(1, 2, E("GG"), 0, 4)], {}, "AGGC"),
        ([D5, D5], [(0, 1, E("T"), 0, 1), (1, 1, E("G"), 0, 1)], {}, "TG"),
        ([A5], [(0, 1, E("T"), 0, 2)], dict(min_count=2), "AT"),
        ([A5], [(0, 1, E("T"), 0, 2)], dict(min_count=3), "A"),
        ([A5], [(0, 1, E("T"), 0, 2)], dict(call_ppm=400000), "AT"),
        ([A5], [(0, 1, E("T"), 0, 2)], dict(call_ppm=400001), "A"),
        ([A5], [(0, 1, E("T"), 0, 2)], dict(min_count=0, min_depth=0), "AT"),
        ([A5], [(0, 1, E("G"), 0, 2), (0, 1, E("T"), 0, 3)], dict(min_count=2), "AT"),
        ([A5], [(0, 32, E("ACGT" * 8), 0, 1)], {}, "A" + "ACGT" * 8),
    ]
    for cols, rows, kw, want in cases:
        planes = np.array(cols, np.uint32).T.copy()
        off, t = install(bc, [(0, 9, 9 + len(cols))], planes, rows)
        got = check_cons(bc, planes, off, t, **kw)
        assert bytes(got.compact(0)).decode() == want, (cols, rows, kw)


def test_consensus_positions(bc, P):
    """Insertions at the first and last position of a segment, at consecutive
    positions, after DEL-called positions, at tile edges."""
    rng = np.random.default_rng(45)
    segs = [(0, 0, 5), (0, 3, P + 10), (1, 0, 0), (1, 7, 2 * P + 1), (2, 0, 1)]
    off = bm.seg_offsets([s[1] for s in segs], [s[2] for s in segs])
    n = int(off[-1])
    planes = random_planes(rng, n, p_empty=0.05)
    index = [off[s] for s in (0, 1, 3, 4)] + [off[s + 1] - 1 for s in (0, 1, 3, 4)]      # first and last positions
    index += list(range(int(off[1]) + 20, int(off[1]) + 30))                             # consecutive positions
    index += [off[1] + P - 4, off[1] + P - 3, off[3] + P - 8, off[3] + P - 7, off[3] + 2 * P - 8]   # around tile edges
    dele = np.flatnonzero((planes[bm.DEL] >= 3) & (planes[:4].max(axis=0) < 3))
    index += dele[::3].tolist()                                                          # DEL-called anchors
    planes[:, int(off[1]) + 24] = (0, 0, 0, 0, 0, 9)
    planes[:, int(off[1]) + 25] = (0, 0, 0, 0, 0, 9)
    rows = random_rows(rng, index)
    off2, t = install(bc, segs, planes, rows)
    assert np.array_equal(off2, off)
    got = check_cons(bc, planes, off, t)
    assert got.inserted[:, 0].sum() > 20 and got.inserted[2].tolist() == [0, 0]
    check_cons(bc, planes, off, t, min_depth=4, min_count=2, call_ppm=300000, iupac=True)
    ref = rng.integers(0, 5, size=n).astype(np.uint8)
    check_cons(bc, planes, off, t, min_depth=3, fill_ref=True, ref=ref)
    # without the flag, on this tracking handle: byte for byte the consensus of before
    plain = bc.consensus(min_depth=3, fill_ref=True, ref=ref)
    first, summary, aligned, compact = cm.consensus_model(planes, off, min_depth=3, fill_ref=True, ref=ref)
    assert plain.inserted is None and np.array_equal(plain.first, first) and np.array_equal(plain.summary, summary)
    assert np.array_equal(bc.consensus_letters(False, 0, n), aligned)
    assert np.array_equal(bc.consensus_letters(True, 0, plain.n), compact)
    assert _code(lambda: _lib.check(bc._lib.mc_bases_consensus_ins(bc._h, _lib.ptr(np.zeros(10, np.int64))),
                                    bc._lib)) == _lib.MC_E_STATE


def test_consensus_every_tile_of_5000(bc):
    """5000 one-position segments (more tiles than one scan iteration), an
    insertion on every one of them."""
    rng = np.random.default_rng(46)
    S = 5000
    segs = [(int(rng.integers(0, N_REF)), i, i + 1) for i in rng.integers(0, 10 ** 6, size=S).tolist()]
    planes = random_planes(rng, S, p_del=0.3)
    off, t = install(bc, segs, planes, random_rows(rng, range(S), max_alleles=2))
    assert bc.timing()["tiles"] == S
    got = check_cons(bc, planes, off, t)
    assert 0 < got.inserted[:, 0].sum() < S and set(got.inserted[:, 0].tolist()) == {0, 1}
    check_cons(bc, planes, off, t, min_count=2, iupac=True)


# --------------------------------------------------------------------- fuzz

@pytest.mark.parametrize("seed", range(20))
def test_fuzz(bc, P, seed):
    rng = np.random.default_rng(700 + seed)
    L = 2 * P + int(rng.integers(0, 50))
    reads = im.random_reads(rng, 600, n_ref=2, length=L, ins_frac=0.05, max_read=150)
    # a few piles with insertions, so that counts above one and competing alleles occur
    for _ in range(40):
        p = int(rng.choice([17, P - 1, P, L - 3]))
        ins = str(rng.choice(["A", "C", "AC", "AC", "N"]))
        reads.append((int(rng.integers(0, 2)), p - 1, "2M%dI1M" % len(ins), "GG" + ins + "T", 30))
    reads.sort(key=lambda r: (r[0], r[1]))
    b = bm.make_batch(reads)
    segs = [(0, 0, L), (1, 0, L)]
    for _ in range(int(rng.integers(0, 3))):
        a = int(rng.integers(0, L))
        segs.append((int(rng.integers(0, 2)), a, a + int(rng.integers(0, L))))
    tids, starts, ends = segments(segs)
    cut = sorted(rng.integers(0, len(reads), size=2).tolist())
    parts = [bm.slice_batch(b, a, z) for a, z in zip([0] + cut, cut + [len(reads)])]
    off = count(bc, segs, parts)
    _, planes = bm.counts_model(b, tids, starts, ends)
    assert np.array_equal(bc.counts(), planes)
    t = im.table_model(b, tids, starts, ends)
    assert len(t["i"]) > 10
    check_table(bc, t, off, planes, [(0, 1, 0), (int(rng.integers(0, 6)), int(rng.integers(0, 4)),
                                                int(rng.integers(0, 400000)))])
    check_cons(bc, planes, off, t, min_depth=int(rng.integers(0, 4)), min_count=int(rng.integers(0, 3)),
               call_ppm=int(rng.integers(0, 500000)), iupac=bool(seed % 3 == 0))


# --------------------------------------------------------------- end to end

_cache = {}


def golden(golden_dir, name):
    if name not in _cache:
        path = os.path.join(golden_dir, name)
        names, lengths, b, _ = bm.kept_reads(path)
        names = [w.split()[0] for w in names]
        segs = [(t, 0, L) for t, L in enumerate(lengths)]
        tids, starts, ends = segments(segs)
        off, planes = bm.counts_model(b, tids, starts, ends)
        _cache[name] = (path, names, segs, off, planes, im.table_model(b, tids, starts, ends))
    return _cache[name]


@pytest.mark.parametrize("name", ["synth_exp.bam", "synth_multi.bam"])
def test_cli_bases_insertions(golden_dir, tmp_path, name):
    from metacov_amd.cli import main
    path, names, segs, off, planes, t = golden(golden_dir, name)
    tids, starts, _ = segments(segs)
    for args, th in (([], (1, 1, 0)), (["--min-depth", "4", "--min-count", "1", "--min-frac", "0.1"], (4, 1, 100000))):
        want = im.tsv(names, tids, starts, off, planes, im.filter_table(t, planes, *th))
        texts = []
        for decode in ("host", "gpu"):
            out, tsv = tmp_path / ("%s.txt" % decode), tmp_path / ("%s.tsv" % decode)
            r = CliRunner().invoke(main, ["bases", "-b", path, "-o", str(out), "--insertions", str(tsv), "--decode",
                                          decode] + args)
            assert r.exit_code == 0, r.output
            texts.append(tsv.read_bytes())
        assert texts[0] == texts[1]
        assert texts[0].decode() == want and want.count("\n") > 3


@pytest.mark.parametrize("name", ["synth_exp.bam", "synth_multi.bam"])
def test_cli_consensus_insertions(golden_dir, tmp_path, name):
    from metacov_amd.cli import main
    path, names, segs, off, planes, t = golden(golden_dir, name)
    first, summary, inserted, aligned, compact = im.consensus_model(planes, off, t, min_depth=2)
    assert inserted[:, 0].sum() > 0
    want = "".join(cm.fasta(names[s], compact[first[s]:first[s + 1]], 60) for s in range(len(segs)))
    want_summary = im.summary_table([(names[t_], a, b, summary[s], inserted[s]) for s, (t_, a, b) in enumerate(segs)])
    texts = []
    for decode in ("host", "gpu"):
        out, tsv = tmp_path / ("%s.fa" % decode), tmp_path / ("%s.tsv" % decode)
        r = CliRunner().invoke(main, ["consensus", "-b", path, "-o", str(out), "--summary", str(tsv), "--decode",
                                      decode, "--insertions", "--min-depth", "2"])
        assert r.exit_code == 0, r.output
        texts.append(out.read_bytes())
        assert tsv.read_text() == want_summary
    assert texts[0] == texts[1] and texts[0].decode() == want
    # the convenience call, and without the flag the summary of before
    big = int(np.argmax([e for _, _, e in segs]))
    got, row = mb.consensus(path, names[big], min_depth=2, insertions=True)
    assert np.array_equal(got, compact[first[big]:first[big + 1]]) and np.array_equal(row, summary[big])
    out, tsv = tmp_path / "plain.fa", tmp_path / "plain.tsv"
    r = CliRunner().invoke(main, ["consensus", "-b", path, "-o", str(out), "--summary", str(tsv), "--min-depth", "2"])
    assert r.exit_code == 0, r.output
    f0, s0, a0, c0 = cm.consensus_model(planes, off, min_depth=2)
    assert tsv.read_text() == cm.summary_table([(names[t_], a, b, s0[s]) for s, (t_, a, b) in enumerate(segs)])
    assert out.read_text() == "".join(cm.fasta(names[s], c0[f0[s]:f0[s + 1]], 60) for s in range(len(segs)))
