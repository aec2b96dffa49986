"""The base-count commands across group boundaries, and the lifetime of the
window-row results.

`bases`, `consensus`, `diversity` and `compare` work through their segments in
groups of at most BASES_GROUP_POSITIONS (COMPARE_GROUP_POSITIONS) positions,
one mc_bases_begin each; at the real limits (2^30, 2^29) no test input reaches
a second group.  Here the limits are lowered to 512 on a BAM of four small
contigs, and every output file must be byte for byte what the same command
writes in one group.  Then the eight accessors of mc_bases_diversity and
mc_bases_compare: MC_E_STATE with their own text before the compute call and
after everything that changes the planes."""
import ctypes
import logging

import numpy as np
import pytest
from click.testing import CliRunner

from metacov_amd import _lib
from metacov_amd import bases as mb
from metacov_amd import cli
from metacov_amd import synth
from tests import bases_model as bm

pytestmark = pytest.mark.gpu

NAMES = ["g_1", "g_2", "g_3", "g_4"]
LENGTHS = [300, 700, 50, 130]           # g_3 has no reads
LIMIT = 512
REGIONS = [(1, 100, 600), (0, 0, 300), (3, 10, 130)]      # 500 | 300 + 120
M, I, D = 0, 1, 2


def _records(rng, ref, bias):
    """About 200 reads on g_1, g_2 and g_4: mismatches (towards `bias`), a few
    insertions and deletions, both strands; on every contig one read starts at
    position 0 and one ends on the last position."""
    recs = []
    for tid in (0, 1, 3):
        L = LENGTHS[tid]
        for i in range(67):
            n = int(rng.integers(20, 61))
            pos = 0 if i == 0 else L - n if i == 1 else int(rng.integers(0, L - n + 1))
            if i % 9 == 4:                  # 2 inserted bases: n - 2 reference positions
                k = int(rng.integers(5, n - 7))
                cigar, span = [(M, k), (I, 2), (M, n - 2 - k)], n - 2
                seq = ref[tid][pos:pos + k] + ("GG", "TT", "GT")[i % 3] + ref[tid][pos + k:pos + span]
            elif i % 9 == 7 and pos + n + 3 <= L:
                k = int(rng.integers(5, n - 5))
                cigar = [(M, k), (D, 3), (M, n - k)]
                seq = ref[tid][pos:pos + k] + ref[tid][pos + k + 3:pos + n + 3]
            else:
                cigar, seq = [(M, n)], ref[tid][pos:pos + n]
            seq = "".join(bias if rng.random() < 0.08 else c for c in seq)
            recs.append(synth.SynthRecord("r%d_%d" % (tid, i), tid, pos, 16 * (i % 2), cigar, n, seq=seq))
    recs.sort(key=lambda r: (r.tid, r.pos))
    return recs


@pytest.fixture(scope="module")
def files(tmp_path_factory, lib_built):
    d = tmp_path_factory.mktemp("groups")
    rng = np.random.default_rng(2024)
    ref = ["".join(rng.choice(list("ACGT"), size=L)) for L in LENGTHS]
    fa = str(d / "ref.fa")
    synth.write_fasta(fa, dict(zip(NAMES, ref)))
    bams = []
    for k, bias in enumerate("AC"):
        path = str(d / ("sample_%s.bam" % "ab"[k]))
        recs = _records(np.random.default_rng(90 + k), ref, bias)
        synth.write_bam(path, NAMES, LENGTHS, recs)
        assert bm.kept_reads(path)[3]["kept"] == len(recs) == 201
        bams.append(path)
    rc = str(d / "regions.csv")
    with open(rc, "w") as fh:
        fh.write("sequence_id,start,stop\n" + "".join("%s,%d,%d\n" % (NAMES[t], a, b) for t, a, b in REGIONS))
    return bams, fa, rc


def test_groups_at_the_lowered_limit():
    assert list(cli.depth_groups(np.zeros(4, np.int64), LENGTHS, LIMIT)) == [(0, 1), (1, 2), (2, 4)]
    starts, ends = [a for _, a, _ in REGIONS], [b for _, _, b in REGIONS]
    assert list(cli.depth_groups(starts, ends, LIMIT)) == [(0, 1), (1, 3)]
    assert list(cli.depth_groups(np.zeros(4, np.int64), LENGTHS, cli.BASES_GROUP_POSITIONS)) == [(0, 4)]
    assert list(cli.depth_groups(np.zeros(4, np.int64), LENGTHS, cli.COMPARE_GROUP_POSITIONS)) == [(0, 4)]


# command, its arguments (AUX: the second output, FA: the reference, B: the second sample), the header of the
# output and of the second output
CASES = {
    "bases": ("bases", [], mb.HEADER, None),
    "bases_all_strand": ("bases", ["--all", "--strand"], mb.HEADER_STRAND, None),
    "bases_quality_insertions": ("bases", ["--quality", "--insertions", "AUX"], mb.HEADER_QUALITY,
                                 mb.INSERTIONS_HEADER),
    "consensus": ("consensus", ["--summary", "AUX", "--insertions", "-f", "FA"], None, mb.SUMMARY_HEADER_INS),
    "diversity": ("diversity", ["--by", "64", "-f", "FA"], mb.DIVERSITY_HEADER, None),
    "compare": ("compare", ["-c", "B", "--by", "64"], mb.COMPARE_HEADER, None),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_grouped_output_is_the_one_group_output(files, tmp_path, monkeypatch, caplog, case):
    (bam_a, bam_b), fa, rc = files
    command, extra, header, aux_header = CASES[case]
    caplog.set_level(logging.INFO)
    begins = []
    begin = mb.BaseCounter.begin
    monkeypatch.setattr(mb.BaseCounter, "begin", lambda self, *a, **kw: (begins.append(1), begin(self, *a, **kw))[1])

    def run(tag, decode, regions):
        out, aux = tmp_path / (tag + ".out"), tmp_path / (tag + ".aux")
        args = [{"AUX": str(aux), "FA": fa, "B": bam_b}.get(x, x) for x in extra]
        caplog.clear()
        del begins[:]
        r = CliRunner().invoke(cli.main, [command, "-b", bam_a, "-o", str(out), "--decode", decode] + args +
                               (["-rc", rc] if regions else []))
        assert r.exit_code == 0, r.output
        logged = [m for m in caplog.messages if "umber of records" in m]
        return out.read_text(), aux.read_text() if aux_header else None, logged, len(begins)

    counters = 2 if command == "compare" else 1
    for decode, regions in (("host", False), ("gpu", False), ("host", True), ("gpu", True)):
        tag = "%s_%d" % (decode, regions)
        whole = run("one_" + tag, decode, regions)
        with monkeypatch.context() as m:
            m.setattr(cli, "BASES_GROUP_POSITIONS", LIMIT)
            m.setattr(cli, "COMPARE_GROUP_POSITIONS", LIMIT)
            grouped = run("grp_" + tag, decode, regions)
        assert whole[3] == counters and grouped[3] == counters * (2 if regions else 3), (tag, whole[3], grouped[3])
        assert grouped[0] == whole[0], tag
        assert grouped[1] == whole[1], tag
        assert len(whole[2]) == counters and grouped[2] == whole[2], tag
        assert "201" in whole[2][0]
        text, aux = grouped[:2]
        if header is not None:
            assert text.startswith(header) and text.count(header) == 1 and len(text) > 2 * len(header)
        else:
            assert text.count(">") == (3 if regions else 4)
        if aux_header is not None:
            assert aux.startswith(aux_header) and aux.count(aux_header) == 1 and len(aux) > len(aux_header)


# ---------------------------------------------------------- result lifetime

TEXTS = {"diversity": "no diversity computed (call mc_bases_diversity)",
         "compare": "no comparison computed (call mc_bases_compare)"}


def _accessors(lib, h, kind):
    first, f32a, f32b = np.zeros(8, np.int64), ctypes.c_float(), ctypes.c_float()
    dp, dn = ctypes.c_void_p(), ctypes.c_int64()

    def fn(name):
        return getattr(lib, "mc_bases_%s_%s" % (kind, name))

    return {"first": lambda: fn("first")(h._h, _lib.ptr(first)),
            "get": lambda: fn("get")(h._h, 0, 0, None),
            "device": lambda: fn("device")(h._h, ctypes.byref(dp), ctypes.byref(dn)),
            "timing": lambda: fn("timing")(h._h, ctypes.byref(f32a), ctypes.byref(f32b))}


def _stale(lib, h, kind):
    for name, call in _accessors(lib, h, kind).items():
        assert call() == _lib.MC_E_STATE, (kind, name)
        assert TEXTS[kind] in lib.mc_last_error().decode(), (kind, name)
    return True


def _fresh(lib, h, kind):
    return all(call() == 0 for call in _accessors(lib, h, kind).values())


def _rows(lib, h, kind, n):
    got = np.zeros((n, 8), np.int64)
    _lib.check(getattr(lib, "mc_bases_%s_get" % kind)(h._h, 0, n, _lib.ptr(got)), lib)
    return got


def test_result_lifetime(lib_built):
    lib = _lib.load()
    rng = np.random.default_rng(5)
    seg = ([0], [0], [200])
    pa, pb = (rng.integers(0, 12, size=(6, 200)).astype(np.uint32) for _ in range(2))
    one_read = bm.batch_args(bm.make_batch([(0, 1, "2M", "CG", 30)]))
    with mb.BaseCounter(1, 0) as h, mb.BaseCounter(1, 0) as o:
        def fill():
            for x, p in ((h, pa), (o, pb)):
                x.begin(*seg)
                x.set_counts(0, p)

        def compute():
            return h.diversity(64).rows.copy(), h.compare(o, 64).rows.copy()

        fill()
        assert _stale(lib, h, "diversity") and _stale(lib, h, "compare")       # before their compute call
        div, cmp = compute()
        assert len(div) == len(cmp) == 4 and div.any() and cmp.any()
        assert _fresh(lib, h, "diversity") and _fresh(lib, h, "compare")
        # each result lives across the other's compute call
        assert np.array_equal(_rows(lib, h, "diversity", 4), div)
        h.diversity(64)
        assert np.array_equal(_rows(lib, h, "compare", 4), cmp)
        # the second handle owns nothing, and nothing that happens to it reaches the first handle's comparison:
        # the rows stay those of the planes it had
        assert _stale(lib, o, "diversity") and _stale(lib, o, "compare")
        o.set_counts(3, np.zeros((6, 2), np.uint32))
        assert np.array_equal(_rows(lib, h, "compare", 4), cmp)
        o.add_reads(*one_read)
        assert np.array_equal(_rows(lib, h, "compare", 4), cmp)
        o.begin([0], [0], [4])
        assert np.array_equal(_rows(lib, h, "compare", 4), cmp) and _fresh(lib, h, "diversity")
        # what changes the first handle's planes drops both results
        for change in (lambda: h.begin(*seg), lambda: h.add_reads(*one_read),
                       lambda: h.set_counts(3, np.zeros((6, 2), np.uint32))):
            fill()
            compute()
            assert _fresh(lib, h, "diversity") and _fresh(lib, h, "compare")
            change()
            assert _stale(lib, h, "diversity") and _stale(lib, h, "compare")
