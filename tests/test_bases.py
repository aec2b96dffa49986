"""Per-position base counts, host side: the test model against a literal loop
and against counts worked out by hand, the host record source against the
model's own BAM reader on every golden file, the table writer's bytes, the
`bases` command's option errors and the ABI table.  No GPU."""
import io
import os
import struct
import zlib

import numpy as np
import pytest
from click.testing import CliRunner

from metacov_amd import _lib
from tests import bases_model as bm
from tests.bases_model import A, C, G, T, N, DEL

ALL_OPS = "2H3S5M2I4M3D6M7N2=1X1P2M4S"       # query 3+5+2+4+6+2+1+2+4 = 29, span 5+4+3+6+7+2+1+2 = 30


# ------------------------------------------------------------------ model

def test_model_by_hand():
    """Every CIGAR op and every nt16 code, counted by hand."""
    bases = "NNNACGTNAAACGTCCCCCCGTANNNN" + "GG"      # 29 bases; S = NNN, then ACGTN | (AA) | ACGT | CCCCCC | GT A GG
    assert len(bases) == bm.query_length(bm.cigar_words(ALL_OPS)) == 29
    assert bm.ref_span(bm.cigar_words(ALL_OPS)) == 30
    b = bm.make_batch([(0, 10, ALL_OPS, bases, 30)])
    off, p = bm.counts_model(b, [0], [0], [50])
    assert off.tolist() == [0, 50]
    want = np.zeros((6, 50), np.uint32)
    for k, ch in enumerate([A, C, G, T, N]):          # 5M at 10
        want[ch, 10 + k] = 1
    for k, ch in enumerate([A, C, G, T]):             # 2I skipped (AA); 4M at 15
        want[ch, 15 + k] = 1
    want[DEL, 19:22] = 1                              # 3D
    want[C, 22:28] = 1                                # 6M
    # 7N: 28..34 nothing; 2= at 35: G T ; 1X at 37: A ; 1P ; 2M at 38: N N ; the last 4S (NNGG) not counted
    want[G, 35] = want[T, 36] = want[A, 37] = 1
    want[N, 38:40] = 1
    assert np.array_equal(p, want)
    assert np.array_equal(bm.counts_loop(b, [0], [0], [50])[1], want)


def test_model_channel_table():
    """nt16 codes 1, 2, 4, 8 are A, C, G, T; every other code, 0 included, is N."""
    b = bm.make_batch([(0, 0, "16M", list(range(16)), 30)])
    _, p = bm.counts_model(b, [0], [0], [16])
    want = [N, A, C, N, G, N, N, N, T] + [N] * 7
    assert [int(np.flatnonzero(p[:, i])[0]) for i in range(16)] == want
    assert p.sum() == 16


def test_model_quality_rule():
    b = bm.make_batch([(0, 0, "2M1D2M", "ACGT", [14, 15, 16, 0]),
                       (0, 0, "4M", "ACGT", None)])                  # qualities absent: passes any threshold
    _, p0 = bm.counts_model(b, [0], [0], [5], 0)
    _, p15 = bm.counts_model(b, [0], [0], [5], 15)
    _, p99 = bm.counts_model(b, [0], [0], [5], 99)
    assert p0.sum(axis=0).tolist() == [2, 2, 2, 2, 1]
    assert p15.sum(axis=0).tolist() == [1, 2, 2, 2, 0]               # Q14 and Q0 drop, DEL stays
    assert p99.sum(axis=0).tolist() == [1, 1, 2, 1, 0]
    assert p99[DEL, 2] == 1


def _random_reads(rng, n_ref=2, n=25, max_pos=90):
    reads = []
    for _ in range(n):
        ops = []
        for _ in range(int(rng.integers(1, 7))):
            ops.append((int(rng.choice([0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8])), int(rng.integers(1, 9))))
        ql = sum(l for op, l in ops if op in bm.QUERY_OPS)
        q = rng.integers(0, 42, size=ql).tolist() if rng.random() < 0.8 else None
        reads.append((int(rng.integers(0, n_ref)), int(rng.integers(0, max_pos)), ops,
                      rng.integers(0, 16, size=ql).tolist(), q))
    reads.sort(key=lambda r: (r[0], r[1]))
    return reads


@pytest.mark.parametrize("seed", range(12))
def test_model_matches_loop(seed):
    rng = np.random.default_rng(seed)
    b = bm.make_batch(_random_reads(rng), seq_gap=seed % 3, qual_gap=seed % 2)
    k = int(rng.integers(1, 6))
    tids = rng.integers(0, 2, size=k)
    starts = rng.integers(0, 100, size=k)
    ends = starts + rng.integers(0, 60, size=k)
    mq = [0, 15, 41][seed % 3]
    a = bm.counts_model(b, tids, starts, ends, mq)
    c = bm.counts_loop(b, tids, starts, ends, mq)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) and a[1].dtype == np.uint32
    # split into batches: the same
    h = bm.n_reads(b) // 2
    d = bm.counts_model([bm.slice_batch(b, 0, h), bm.slice_batch(b, h, bm.n_reads(b))], tids, starts, ends, mq)
    assert np.array_equal(a[1], d[1])


def test_model_at_the_int32_edge(lib_built):
    """bases_model.int32_edge_case (the GPU tests' read set around 2^31 and
    below 2^32): the numpy model against the literal loop, in one and in two
    batches, and the positions the sites model reports."""
    from metacov_amd import bases as mb
    P = mb.dims()
    reads, segs, scrambled, k = bm.int32_edge_case(P)
    b = bm.make_batch(reads)
    assert b["pos"].dtype == np.int32 and int(b["pos"].max()) == 2 ** 31 - 1 and 0 < k < bm.n_reads(b)
    for sg in (segs, scrambled):
        tids, starts, ends = (np.array(x, np.int64) for x in zip(*sg))
        a = bm.counts_model(b, tids, starts, ends)
        c = bm.counts_loop(b, tids, starts, ends)
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
        for s in range(len(sg)):                                          # every segment holds counts
            assert a[1][:, a[0][s]:a[0][s + 1]].sum() > 0, sg[s]
        d = bm.counts_model([bm.slice_batch(b, 0, k), bm.slice_batch(b, k, bm.n_reads(b))], tids, starts, ends)
        assert np.array_equal(a[1], d[1])
        first, pos, cnt = bm.sites_model(a[1], a[0], starts, 0, 0, 0)
        assert pos.dtype == np.int64
        assert np.array_equal(pos, np.concatenate([np.arange(x, y, dtype=np.int64) for x, y in zip(starts, ends)]))
        first, pos, cnt = bm.sites_model(a[1], a[0], starts, 1, 1, 0)
        assert pos.max() > 2 ** 31 + 2 ** 30 and (pos == 2 ** 31 - 1).sum() >= 2 and (pos < 400).any()
        for s in range(len(sg)):
            p = pos[first[s]:first[s + 1]]
            assert ((p >= starts[s]) & (p < ends[s])).all() and (np.diff(p) > 0).all()
            assert np.array_equal(cnt[first[s]:first[s + 1]].T, a[1][:, a[0][s] + p - starts[s]])


def test_sites_model_by_hand():
    #            A   C   G   T   N  DEL
    cols = [(10,  0,  0,  0,  5,  0),      # no alt
            (10,  2,  0,  0,  0,  0),      # alt 2 of 12
            (5,   5,  0,  0,  0,  0),      # tie: base A (lowest), alt 5
            (0,   0,  0,  9,  0,  1),      # alt = DEL 1 of 10
            (0,   0,  0,  0,  7,  0),      # only N: depth 0
            (0,   3,  0,  0,  0,  0)]      # major allele C
    planes = np.array(cols, np.uint32).T
    first, pos, cnt = bm.sites_model(planes, [0, 4, 4, 6], [100, 7, 0], 1, 1, 0)
    assert (first.tolist(), pos.tolist()) == ([0, 3, 3, 3], [101, 102, 103])
    assert cnt.tolist() == [list(cols[1]), list(cols[2]), list(cols[3])]
    # alt * 10^6 >= min_ppm * depth: 2 / 12 = 166 666.67 ppm
    assert bm.sites_model(planes, [0, 6], [0], 1, 1, 166666)[1].tolist() == [1, 2]
    assert bm.sites_model(planes, [0, 6], [0], 1, 1, 166667)[1].tolist() == [2]
    assert bm.sites_model(planes, [0, 6], [0], 11, 1, 0)[1].tolist() == [1]
    # with a reference: position 5 (only C) against ref A is a site; ref code 4 falls back to the major allele
    ref = np.array([0, 0, 1, 4, 4, 0], np.uint8)
    assert bm.sites_model(planes, [0, 6], [0], 1, 1, 0, ref)[1].tolist() == [1, 2, 3, 5]
    # thresholds of zero: every position
    assert bm.sites_model(planes, [0, 6], [0], 0, 0, 0)[1].tolist() == [0, 1, 2, 3, 4, 5]


# ------------------------------------------------------------- record source

def _source_batches(path, max_reads=1 << 20, max_bases=1 << 27, **kw):
    from metacov_amd.bases import BaseSource
    out = []
    with BaseSource(path, 2, **kw) as src:
        while True:
            b = src.next(max_reads, max_bases)
            if b is None:
                break
            out.append({k: v.copy() for k, v in b.items()})
        return src.references, src.lengths, out, src.counts()


def _same_reads(batches, want):
    i = 0
    for b in batches:
        n = bm.n_reads(b)
        w = bm.slice_batch(want, i, i + n)
        for k in ("tid", "pos", "l_seq", "cig_off", "cigar", "seq_off", "seq", "qual_off", "qual"):
            assert b[k].dtype == w[k].dtype and np.array_equal(b[k], w[k]), k
        i += n
    assert i == bm.n_reads(want)


GOLDEN_COUNTS = {"bbmap.sorted.bam": (3979, 0, 0), "synth_exp.bam": (725, 0, 0),
                 "synth_exp_noseq.bam": (None, 1, 0), "synth_edge.bam": (9635, 0, 15),
                 "synth_multi.bam": (5797, 0, 17), "synth_longcigar.bam": (None, 0, 0)}


@pytest.mark.parametrize("name", sorted(GOLDEN_COUNTS))
def test_source_equals_model_reader(lib_built, golden_dir, name):
    path = os.path.join(golden_dir, name)
    names, lengths, want, counts = bm.kept_reads(path)
    refs, lens, got, got_counts = _source_batches(path)
    assert [r.split()[0] for r in refs] == names and list(lens) == lengths
    assert got_counts == counts
    kept, no_seq, bad = GOLDEN_COUNTS[name]
    assert (counts["no_seq"], counts["bad_cigar"]) == (no_seq, bad)
    if kept is not None:
        assert counts["kept"] == kept
    _same_reads(got, want)
    assert bm.n_reads(want) == counts["kept"] - no_seq - bad
    # small batches, by reads and by bases: the same reads in the same order
    _same_reads(_source_batches(path, max_reads=97)[2], want)
    _same_reads(_source_batches(path, max_bases=1000)[2], want)


def test_source_noseq_two_records(lib_built, golden_dir):
    c = _source_batches(os.path.join(golden_dir, "synth_exp_noseq.bam"))[3]
    assert c["no_seq"] == 1 and c["kept"] == 2


def test_source_long_cigar(lib_built, golden_dir):
    _, _, got, _ = _source_batches(os.path.join(golden_dir, "synth_longcigar.bam"))
    n_ops = np.concatenate([np.diff(b["cig_off"]) for b in got])
    assert n_ops.sum() == 140001 and n_ops.max() == 140000      # the CG:B,I tag, not the 2-op placeholder


def test_source_filters(lib_built, golden_dir):
    """MAPQ 9..44 and Q15 both discriminate on bbmap.sorted.bam."""
    path = os.path.join(golden_dir, "bbmap.sorted.bam")
    _, _, want, counts = bm.kept_reads(path)
    assert int(want["l_seq"].sum()) == 343279
    low = sum(int((want["qual"][int(want["qual_off"][i]):int(want["qual_off"][i + 1])] < 15).sum())
              for i in range(bm.n_reads(want)))
    assert low == 5938
    _, _, w30, c30 = bm.kept_reads(path, min_mapq=30)
    assert 0 < c30["kept"] < counts["kept"]
    _, _, got, got_c = _source_batches(path, min_mapq=30)
    assert got_c == c30
    _same_reads(got, w30)
    _, _, wf, cf = bm.kept_reads(path, flag_filter=0x714)
    _, _, got, got_c = _source_batches(path, flag_filter=0x714)
    assert got_c == cf and 0 < cf["kept"] < counts["kept"]
    _same_reads(got, wf)


def test_source_small_windows(lib_built, golden_dir, monkeypatch):
    """Records that straddle inflate windows are carried over whole."""
    path = os.path.join(golden_dir, "synth_multi.bam")
    want = bm.kept_reads(path)[2]
    monkeypatch.setenv("MC_BASES_WINDOW", "1")       # one BGZF block per window
    _same_reads(_source_batches(path)[2], want)


def _bgzf(payload):
    def block(data):
        comp = zlib.compressobj(6, zlib.DEFLATED, -15)
        c = comp.compress(data) + comp.flush()
        head = struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(c) + 25)
        return head + c + struct.pack("<II", zlib.crc32(data), len(data))
    return block(payload) + block(b"")


def _bam_bytes(records, n_ref=1):
    out = b"BAM\1" + struct.pack("<i", 0) + struct.pack("<i", n_ref)
    for t in range(n_ref):
        name = b"c%d\0" % t
        out += struct.pack("<i", len(name)) + name + struct.pack("<i", 1000)
    for tid, pos in records:
        body = struct.pack("<iiBBHHHiiii", tid, pos, 2, 30, 0, 1, 0, 4, -1, -1, 0) + b"r\0" + \
            struct.pack("<I", 4 << 4) + bytes([0x12, 0x48]) + bytes([30] * 4)
        out += struct.pack("<i", len(body)) + body
    return out


def test_source_unsorted_file(lib_built, tmp_path):
    from metacov_amd.bases import BaseSource
    good = tmp_path / "good.bam"
    good.write_bytes(_bgzf(_bam_bytes([(0, 5), (0, 5), (0, 9)])))
    with BaseSource(str(good)) as src:
        b = src.next()
        assert b["pos"].tolist() == [5, 5, 9] and b["seq"].tolist() == [0x12, 0x48, 0, 0] * 3
    bad = tmp_path / "bad.bam"
    bad.write_bytes(_bgzf(_bam_bytes([(0, 5), (0, 4)])))
    with BaseSource(str(bad)) as src:
        with pytest.raises(_lib.MetacovError, match="out of order") as e:
            src.next()
        assert e.value.code == _lib.MC_E_INVALID


# ------------------------------------------------------------------ writer

def test_write_sites_bytes():
    from metacov_amd import bases as mb
    fh = io.StringIO()
    n = mb.write_sites(fh, "c1", [0, 41], [[1, 2, 3, 4, 5, 6], [0, 0, 0, 0, 9, 0]])
    assert n == 2
    assert fh.getvalue() == "c1\t1\t.\t16\t1\t2\t3\t4\t5\t6\nc1\t42\t.\t0\t0\t0\t0\t0\t9\t0\n"
    fh = io.StringIO()
    mb.write_sites(fh, "c 2", [7], [[4000000000, 1, 0, 0, 0, 4000000000]], ref=np.frombuffer(b"g", np.uint8))
    assert fh.getvalue() == "c 2\t8\tG\t8000000001\t4000000000\t1\t0\t0\t0\t4000000000\n"
    fh = io.StringIO()
    assert mb.write_sites(fh, "c", [], np.zeros((0, 6))) == 0 and fh.getvalue() == ""
    assert mb.HEADER == "contig\tpos\tref\tdepth\tA\tC\tG\tT\tN\tDEL\n"
    assert mb.ref_codes(np.frombuffer(b"ACGTacgtNn-", np.uint8)).tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 4, 4, 4]
    # the model's table agrees with the writer
    fh = io.StringIO()
    fh.write(mb.HEADER)
    mb.write_sites(fh, "c1", [0, 2], [[1, 2, 3, 4, 5, 6], [7, 0, 0, 0, 0, 0]], ref=np.frombuffer(b"aN", np.uint8))
    assert fh.getvalue() == bm.table({0: "c1"}, [(0, 0, [1, 2, 3, 4, 5, 6]), (0, 2, [7, 0, 0, 0, 0, 0])],
                                     {"c1": "acN"})


# --------------------------------------------------------------------- CLI

@pytest.mark.parametrize("args, match", [
    (["--min-frac", "1.5"], "min-frac"),
    (["--min-frac", "-0.1"], "min-frac"),
    (["--min-frac", "nan"], "min-frac"),
    (["--min-depth", "-1"], "min-depth"),
    (["--min-count", "-1"], "min-count"),
    (["--min-baseq", "-1"], "min-baseq"),
    (["--min-mapq", "-1"], "min-mapq"),
])
def test_cli_option_errors(golden_dir, args, match):
    from metacov_amd.cli import main
    r = CliRunner().invoke(main, ["bases", "-b", os.path.join(golden_dir, "synth_exp.bam")] + args)
    assert r.exit_code == 2 and match in r.output


def test_cli_world_size_and_help(golden_dir, monkeypatch):
    from metacov_amd.cli import main
    monkeypatch.setenv("WORLD_SIZE", "2")
    r = CliRunner().invoke(main, ["bases", "-b", os.path.join(golden_dir, "synth_exp.bam")])
    assert r.exit_code == 2 and "one process" in r.output
    r = CliRunner().invoke(main, ["bases", "--help"])
    assert r.exit_code == 0 and "1-based" in r.output and "--all" in r.output


def test_abi_table_has_bases():
    for name in ("mc_bases_create", "mc_bases_begin", "mc_bases_add_batch", "mc_bases_get", "mc_bases_sites",
                 "mc_bases_sites_get", "mc_bases_dims", "mc_bases_src_open", "mc_bases_src_next",
                 "mc_bases_src_counts"):
        assert name in _lib.SIGNATURES


def test_contig_names():
    from metacov_amd import bases as mb
    assert mb.contig_names(["a b", "", " ", "c_1", "x\ty z"]) == ["a", "", " ", "c_1", "x"]
    assert mb.contig_names([]) == []


def test_one_call_argument_errors(monkeypatch):
    """The one-call functions' contig, range and reference errors, raised from
    the header alone (a stand-in source: no file, no library)."""
    from metacov_amd import bases as mb

    class Header:
        references, lengths = ["ctg_1 first", "ctg_2"], [100, 40]

        def __init__(self, *a):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            pass

    monkeypatch.setattr(mb, "BaseSource", Header)
    monkeypatch.setattr(mb._lib, "load", lambda: None)
    with pytest.raises(KeyError, match="contig 'ctg_3' is not in the header of x.bam"):
        mb.count_coverage("x.bam", "ctg_3")
    with pytest.raises(KeyError, match="contig 'ctg_1 first' is not in the header of x.bam"):
        mb.count_coverage("x.bam", "ctg_1 first")           # the contig id is the name's first word
    for start, stop, text in ((-1, 5, r"bad range \[-1, 5\)"), (7, 6, r"bad range \[7, 6\)")):
        with pytest.raises(ValueError, match=text):
            mb.count_coverage("x.bam", "ctg_1", start, stop)
        with pytest.raises(ValueError, match=text):
            mb.compare("x.bam", "y.bam", "ctg_1", start, stop)
    with pytest.raises(ValueError, match="bad range"):
        mb.diversity("x.bam", "ctg_2", 41)                  # the default stop is the contig's length
    for call in (mb.diversity, mb.consensus):
        with pytest.raises(ValueError, match="ref must have stop - start letters"):
            call("x.bam", "ctg_2", 10, 14, ref="ACG")
        with pytest.raises(ValueError, match="ref must have stop - start letters"):
            call("x.bam", "ctg_2", ref=np.zeros(41, np.uint8))
