"""The GPU decoder's bases mode and the base counter's device batches: the
resident read table against the test model's BAM reader and the host source,
field for field; planes from device batches against planes from the host
path; the errors; `bases --decode gpu` against `--decode host`, byte for byte."""
import ctypes
import os
import struct

import numpy as np
import pytest
from click.testing import CliRunner

from metacov_amd import _lib, synth
from metacov_amd import bases as mb
from metacov_amd.synth import SynthRecord
from tests import bases_model as bm

pytestmark = pytest.mark.gpu

KEYS = ("tid", "pos", "l_seq", "cig_off", "cigar", "seq_off", "seq", "qual_off", "qual")
GOLDENS = ["bbmap.sorted.bam", "synth_edge.bam", "synth_exp.bam", "synth_exp_noseq.bam", "synth_longcigar.bam",
           "synth_multi.bam"]
M, I, D, N, S = 0, 1, 2, 3, 4


def same_table(got, want):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype, k
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        bad = np.flatnonzero(got[k] != want[k])
        assert len(bad) == 0, "%s differs first at %d: got %s, want %s" % (k, bad[0], got[k][bad[0]], want[k][bad[0]])


def host_table(path, **kw):
    """The host source's batches as one table (offsets rebased), and its counts."""
    parts = {k: [] for k in KEYS}
    base = {"cig_off": 0, "seq_off": 0, "qual_off": 0}
    with mb.BaseSource(path, 2, **kw) as src:
        while True:
            b = src.next(4096, 1 << 27)
            if b is None:
                break
            for k in KEYS:
                if k in base:
                    parts[k].append(b[k][:-1] + base[k])
                else:
                    parts[k].append(b[k].copy())
            for k in base:
                base[k] += int(b[k][-1])
        counts = src.counts()
    out = {k: np.concatenate(parts[k] + [np.zeros(0, parts[k][0].dtype if parts[k] else np.int64)]) for k in KEYS}
    for k in base:
        out[k] = np.append(out[k], base[k]).astype(np.int64)
    for k, dt in (("tid", np.int32), ("pos", np.int32), ("l_seq", np.int32), ("cigar", np.uint32),
                  ("seq", np.uint8), ("qual", np.uint8)):
        out[k] = out[k].astype(dt)
    return out, counts


def planes_of(n_ref, segs, feed, min_baseq=0):
    tids, starts, ends = (np.array(x, np.int64) for x in zip(*segs))
    with mb.BaseCounter(n_ref, 0) as h:
        h.begin(tids, starts, ends, min_baseq=min_baseq)
        feed(h)
        return h.counts()


def whole(lengths):
    return [(t, 0, L) for t, L in enumerate(lengths)]


# --------------------------------------------------------------------- goldens

@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("window", [0, 1 << 20])
def test_goldens(lib_built, golden_dir, name, window):
    path = os.path.join(golden_dir, name)
    names, lengths, want, counts = bm.kept_reads(path)
    with mb.GpuBaseSource(path, 0, window_bytes=window) as src:
        assert [r.split()[0] for r in src.references] == names and list(src.lengths) == lengths
        assert src.counts() == counts and len(src) == bm.n_reads(want)
        same_table(src.copy(), want)
        t = src.timings()
        assert t["blocks"] > 0 and t["inflated_bytes"] > 0 and t["windows"] >= (1 if window else 0)
    if name == "synth_longcigar.bam":
        assert int(np.diff(want["cig_off"]).max()) == 140000


def test_filters(lib_built, golden_dir):
    path = os.path.join(golden_dir, "bbmap.sorted.bam")
    counts = bm.kept_reads(path)[3]
    for kw in ({"min_mapq": 30}, {"flag_filter": 0x714}):
        _, _, want, c = bm.kept_reads(path, **kw)
        assert 0 < c["kept"] < counts["kept"]
        with mb.GpuBaseSource(path, 0, **kw) as src:
            assert src.counts() == c
            same_table(src.copy(), want)


# ------------------------------------------------------------- alignment sweep

def write_records(path, names, lengths, bodies):
    """A BAM of already encoded records (synth.write_bam's framing)."""
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % z for z in zip(names, lengths))
    out = bytearray(b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(names)))
    for n, L in zip(names, lengths):
        out += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", int(L))
    for b in bodies:
        out += b
    with open(path, "wb") as fh:
        fh.write(synth._bgzf(bytes(out)))


def test_alignment_sweep(lib_built, tmp_path):
    """l_seq 1..9 x name lengths 1..4: 0..3 padding bytes behind the bases and
    CIGAR, SEQ and QUAL at every source alignment; distinct bases and
    qualities everywhere, one read without qualities (0xFF)."""
    rng = np.random.default_rng(5)
    bodies, srcs = [], set()
    at = 0
    for k, (l, nl) in enumerate((l, nl) for l in range(1, 10) for nl in range(1, 5)):
        cigar = [(M, l)] if l < 4 else [(S, 1), (M, l - 3), (I, 1), (M, 1)]
        seq = "".join(rng.choice(list("ACGTN"), size=l))
        rec = bytearray(synth.encode_record(SynthRecord("abcd"[:nl], 0, 10 + 3 * k, 0, cigar, l, seq=seq)))
        q_at = 4 + 32 + nl + 1 + 4 * len(cigar) + (l + 1) // 2
        rec[q_at:q_at + l] = bytes([0xFF] * l) if k == 17 else bytes((7 * k + j) % 94 for j in range(l))
        srcs.add(((at + 4 + 32 + nl + 1) % 4, (at + q_at - (l + 1) // 2) % 4, (at + q_at) % 4))
        at += len(rec)
        bodies.append(bytes(rec))
    assert {s[0] for s in srcs} == {s[1] for s in srcs} == {s[2] for s in srcs} == {0, 1, 2, 3}
    path = str(tmp_path / "sweep.bam")
    write_records(path, ["c"], [500], bodies)
    _, _, want, counts = bm.kept_reads(path)
    assert bm.n_reads(want) == 36 and set((np.diff(want["seq_off"]) - (want["l_seq"] + 1) // 2).tolist()) == {0, 1, 2, 3}
    assert set((want["qual_off"][:-1] % 4).tolist()) == {0, 1, 2, 3} and (want["qual"] == 0xFF).sum() == 5
    with mb.GpuBaseSource(path, 0) as src:
        assert src.counts() == counts
        same_table(src.copy(), want)
        got = planes_of(1, [(0, 0, 500)], lambda h: h.add_device(src), min_baseq=20)
    assert np.array_equal(got, bm.counts_model(want, [0], [0], [500], 20)[1]) and got.sum() > 0


def test_empty_and_single(lib_built, tmp_path):
    empty = str(tmp_path / "empty.bam")
    synth.write_bam(empty, ["c1", "c2"], [100, 200], [])
    with mb.GpuBaseSource(empty, 0) as src:
        assert list(src.references) == ["c1", "c2"] and len(src) == 0
        assert src.counts() == {"records": 0, "kept": 0, "no_seq": 0, "bad_cigar": 0}
        t = src.copy()
        assert all(len(t[k]) == 0 for k in ("tid", "cigar", "seq", "qual")) and t["cig_off"].tolist() == [0]
        got = planes_of(2, [(0, 0, 100)], lambda h: h.add_device(src))
        assert got.sum() == 0
    one = str(tmp_path / "one.bam")
    synth.write_bam(one, ["c1"], [100], [SynthRecord("r", 0, 7, 0, [(M, 5)], 5, seq="ACGTA")])
    want = bm.kept_reads(one)[2]
    with mb.GpuBaseSource(one, 0) as src:
        same_table(src.copy(), want)
        assert src.copy()["seq"].tolist() == [0x12, 0x48, 0x10, 0]


# ------------------------------------------------------- segments and windows

@pytest.fixture(scope="module")
def big(lib_built, tmp_path_factory):
    """50 000 reads over 3 contigs, about 200 parse segments; the host
    source's table and the host path's planes, computed once."""
    lengths = [40000, 25000, 60000]
    names = ["k1", "k2", "k3"]
    path = str(tmp_path_factory.mktemp("bases_decode") / "big.bam")
    synth.write_bam_fast(path, names, lengths, *synth.edge_mix_arrays(lengths, 50000, seed=11), level=1)
    table, counts = host_table(path)
    planes = planes_of(3, whole(lengths), lambda h: h.add_bam(path))
    return path, lengths, table, counts, planes


@pytest.mark.parametrize("window", [0, 1 << 20])
def test_segments_and_windows(big, window):
    path, lengths, want, counts, _ = big
    with mb.GpuBaseSource(path, 0, window_bytes=window) as src:
        t = src.timings()
        assert t["inflated_bytes"] > 150 * (64 << 10)            # well over a hundred 64 KiB segments
        assert t["resyncs"] <= 64
        if window:
            assert t["windows"] >= 8                             # records straddle the window ends
        assert src.counts() == counts and 0 < counts["kept"] < counts["records"]
        same_table(src.copy(), want)


# ---------------------------------------------------------------- device batches

@pytest.mark.parametrize("name", ["bbmap.sorted.bam", "synth_multi.bam"])
def test_add_device_equals_host_path(lib_built, golden_dir, name):
    path = os.path.join(golden_dir, name)
    lengths = bm.kept_reads(path)[1]
    want = planes_of(len(lengths), whole(lengths), lambda h: h.add_bam(path))
    assert want.sum() > 0
    with mb.GpuBaseSource(path, 0) as src:
        assert np.array_equal(planes_of(len(lengths), whole(lengths), lambda h: h.add_device(src)), want)
        # sub-ranges cut inside piles
        assert np.array_equal(planes_of(len(lengths), whole(lengths), lambda h: h.add_device(src, max_reads=97)),
                              want)
    got = planes_of(len(lengths), whole(lengths), lambda h: h.add_bam(path, decode="gpu"))
    assert np.array_equal(got, want)


def test_add_device_big(big):
    path, lengths, _, counts, want = big
    with mb.GpuBaseSource(path, 0, window_bytes=1 << 20) as src:
        assert np.array_equal(planes_of(3, whole(lengths), lambda h: h.add_device(src)), want)
        assert np.array_equal(planes_of(3, whole(lengths), lambda h: h.add_device(src, max_reads=4099)), want)


def test_two_begins_one_source(lib_built, golden_dir):
    path = os.path.join(golden_dir, "bbmap.sorted.bam")
    _, lengths, b, _ = bm.kept_reads(path)
    t = int(np.argmax(np.bincount(b["tid"])))
    groups =[whole(lengths)[::-1], [(t, 10, lengths[t] // 2), (t, 0, lengths[t])]]
    with mb.GpuBaseSource(path, 0) as src, mb.BaseCounter(len(lengths), 0) as h:
        for segs in groups:
            tids, starts, ends = (np.array(x, np.int64) for x in zip(*segs))
            h.begin(tids, starts, ends)
            h.add_device(src)
            got = h.counts()
            assert got.sum() > 0
            assert np.array_equal(got, planes_of(len(lengths), segs, lambda c: c.add_bam(path)))
        assert h.timing()["reads"] == len(src)


def test_min_baseq(lib_built, golden_dir):
    path = os.path.join(golden_dir, "bbmap.sorted.bam")
    lengths = bm.kept_reads(path)[1]
    want = planes_of(len(lengths), whole(lengths), lambda h: h.add_bam(path), min_baseq=15)
    with mb.GpuBaseSource(path, 0) as src:
        got = planes_of(len(lengths), whole(lengths), lambda h: h.add_device(src), min_baseq=15)
        all_q = planes_of(len(lengths), whole(lengths), lambda h: h.add_device(src))
    assert np.array_equal(got, want) and got.sum() < all_q.sum()


# ----------------------------------------------------------------------- errors

def test_unsorted_file(lib_built, tmp_path):
    path = str(tmp_path / "unsorted.bam")
    recs = [SynthRecord("r%d" % k, 0, p, 0, [(M, 6)], 6, seq="ACGTAC") for k, p in enumerate([5, 9, 8, 20])]
    synth.write_bam(path, ["c"], [100], recs)
    with mb.GpuBaseSource(path, 0) as src, mb.BaseCounter(1, 0) as h:
        assert len(src) == 4                                  # the decode does not check the order
        h.begin([0], [0], [100])
        with pytest.raises(_lib.MetacovError, match="read 2: reads are not sorted") as e:
            h.add_device(src)
        assert e.value.code == _lib.MC_E_INVALID
        assert h.counts().sum() == 0                          # the batch added nothing
        # across sub-ranges: the first read of a batch against the last one of the batch before
        h.begin([0], [0], [100])
        with pytest.raises(_lib.MetacovError, match="read 0: reads are not sorted.*previous batch") as e:
            h.add_device(src, max_reads=2)
        assert e.value.code == _lib.MC_E_INVALID
        assert h.counts().sum() == 12                         # the first sub-range stays
    with mb.BaseCounter(1, 0) as h:
        h.begin([0], [0], [100])
        with pytest.raises(_lib.MetacovError, match="not sorted"):
            h.add_bam(path, decode="gpu")


def test_state_errors(lib_built, golden_dir):
    lib = _lib.load()
    path = os.path.join(golden_dir, "synth_exp.bam")
    n = ctypes.c_int64()
    p = [ctypes.c_void_p() for _ in range(9)]
    r = ctypes.byref
    with mb.GpuBaseSource(path, 0) as src:
        with mb.BaseCounter(len(src.references), 0) as h:
            with pytest.raises(_lib.MetacovError, match="mc_bases_begin") as e:
                h.add_device(src)
            assert e.value.code == _lib.MC_E_STATE
        assert lib.mc_bam_gpu_scan_device(src._h, r(n), *[r(x) for x in p[:7]], r(n)) == _lib.MC_E_STATE
        assert lib.mc_bam_gpu_intervals_device(src._h, r(n), r(p[0]), r(p[1]), r(p[2])) == _lib.MC_E_STATE
        assert lib.mc_bam_gpu_reads_device(src._h, r(n), *[r(x) for x in p], r(n)) == _lib.MC_E_STATE
    g = ctypes.c_void_p()
    _lib.check(lib.mc_bam_gpu_open_scan(path.encode(), 0, 0, 0, r(g)), lib)
    try:
        c = [ctypes.c_int64() for _ in range(4)]
        assert lib.mc_bam_gpu_bases_counts(g, *[r(x) for x in c]) == _lib.MC_E_STATE
        assert lib.mc_bam_gpu_bases_device(g, r(n), r(p[0]), r(p[1]), r(p[2]), r(p[3]), r(n), r(p[4]), r(p[5]),
                                           r(p[6]), r(n), r(p[7]), r(p[8]), r(n)) == _lib.MC_E_STATE
        one = np.zeros(1, np.int64)
        assert lib.mc_bam_gpu_bases_copy(g, None, None, _lib.ptr(one), None, None, _lib.ptr(one), None,
                                         _lib.ptr(one), None) == _lib.MC_E_STATE
    finally:
        lib.mc_bam_gpu_close(g)


# ------------------------------------------------------------------- end to end

def test_cli_decode_gpu_equals_host(lib_built, golden_dir, tmp_path):
    from metacov_amd.cli import main
    path = os.path.join(golden_dir, "bbmap.sorted.bam")
    fa = os.path.join(golden_dir, "reference_1K.fa.gz")
    names, lengths = bm.kept_reads(path)[:2]
    t = int(np.argmax(lengths))
    rc = tmp_path / "r.csv"
    rc.write_text("sequence_id,start,stop\n%s,%d,%d\n%s,0,%d\n" % (names[t], 10, lengths[t] // 2, names[0],
                                                                  lengths[0]))
    for k, args in enumerate((["--all"], ["-f", fa, "--min-depth", "4", "--min-count", "2"],
                              ["--all", "-f", fa, "-rc", str(rc)], ["--min-baseq", "15", "--min-mapq", "30"])):
        out = {}
        for decode in ("host", "gpu"):
            o = tmp_path / ("%d_%s.tsv" % (k, decode))
            res = CliRunner().invoke(main, ["bases", "-b", path, "-o", str(o), "--decode", decode] + args)
            assert res.exit_code == 0, res.output
            out[decode] = o.read_bytes()
        assert out["gpu"] == out["host"] and out["host"].count(b"\n") > 1, args


def test_count_coverage_decode_gpu(lib_built, golden_dir):
    path = os.path.join(golden_dir, "bbmap.sorted.bam")
    names, lengths, b, _ = bm.kept_reads(path)
    t = int(np.argmax(np.bincount(b["tid"])))
    for args in ((), (10, lengths[t] // 2)):
        want = mb.count_coverage(path, names[t], *args)
        got = mb.count_coverage(path, names[t], *args, decode="gpu")
        assert sum(int(w.sum()) for w in want) > 0
        assert all(g.dtype == np.uint32 and np.array_equal(g, w) for g, w in zip(got, want))
