"""The GPU decoder's bases mode, host side: the record rule (mc::gz::rec_bases
through mc_bam_rec_bases_host) against the test model's BAM reader on every
golden file and on records made by hand, every truncation of a record (also
as a stand-alone program under host AddressSanitizer), the ABI table and the
`bases --decode` option.  No GPU."""
import ctypes
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest
from click.testing import CliRunner

from metacov_amd import _lib, synth
from metacov_amd.synth import SynthRecord
from tests import bases_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = ["bbmap.sorted.bam", "synth_edge.bam", "synth_exp.bam", "synth_exp_noseq.bam", "synth_longcigar.bam",
           "synth_multi.bam"]
DROPPED, TAKEN, NO_SEQ, BAD_CIGAR, MALFORMED = range(5)
M, I, D, N, S = 0, 1, 2, 3, 4


def record_bodies(path):
    """(n_ref, [record body bytes]) of a BAM: the bytes after each block_size."""
    with gzip.open(path, "rb") as fh:
        d = fh.read()
    l_text, = struct.unpack_from("<i", d, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", d, o)
    o += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", d, o)
        o += 8 + l_name
    out = []
    while o + 4 <= len(d):
        bs, = struct.unpack_from("<i", d, o)
        out.append(d[o + 4:o + 4 + bs])
        o += 4 + bs
    return n_ref, out


def rule(lib, body, n_ref, flag_filter=0x704, min_mapq=0, length=None):
    """(class, out7) of one record body; the buffer is exactly `length` bytes."""
    length = len(body) if length is None else length
    buf = (ctypes.c_uint8 * max(length, 1)).from_buffer_copy(bytes(body[:length]) or b"\0")
    out = (ctypes.c_int64 * 7)()
    rc = lib.mc_bam_rec_bases_host(ctypes.addressof(buf), length, n_ref, flag_filter, min_mapq, out)
    assert 0 <= rc <= 4, _lib.load().mc_last_error()
    return rc, list(out)


def batch_by_rule(lib, path, **kw):
    """The file's read table and counts, built from the rule's answers alone."""
    n_ref, bodies = record_bodies(path)
    counts = {"records": len(bodies), "kept": 0, "no_seq": 0, "bad_cigar": 0}
    tid, pos, ls, cig, cig_off, seq, seq_off, qual, qual_off = [], [], [], [], [0], bytearray(), [0], bytearray(), [0]
    for body in bodies:
        rc, (t, p, l, nc, c_at, s_at, q_at) = rule(lib, body, n_ref, **kw)
        assert rc != MALFORMED
        if rc == DROPPED:
            continue
        counts["kept"] += 1
        if rc == NO_SEQ:
            counts["no_seq"] += 1
        elif rc == BAD_CIGAR:
            counts["bad_cigar"] += 1
        if rc != TAKEN:
            continue
        assert 32 <= c_at and c_at + 4 * nc <= len(body) and s_at + (l + 1) // 2 == q_at and q_at + l <= len(body)
        tid.append(t)
        pos.append(p)
        ls.append(l)
        cig.append(np.frombuffer(body, "<u4", nc, c_at).astype(np.uint32))
        cig_off.append(cig_off[-1] + nc)
        seq.extend(body[s_at:s_at + (l + 1) // 2])
        seq.extend(b"\0" * (-len(seq) % 4))
        seq_off.append(len(seq))
        qual.extend(body[q_at:q_at + l])
        qual_off.append(len(qual))
    batch = {"tid": np.array(tid, np.int32), "pos": np.array(pos, np.int32), "l_seq": np.array(ls, np.int32),
             "cig_off": np.array(cig_off, np.int64),
             "cigar": np.concatenate(cig + [np.zeros(0, np.uint32)]).astype(np.uint32),
             "seq_off": np.array(seq_off, np.int64), "seq": np.frombuffer(bytes(seq), np.uint8).copy(),
             "qual_off": np.array(qual_off, np.int64), "qual": np.frombuffer(bytes(qual), np.uint8).copy()}
    return batch, counts


def same_batch(got, want):
    for k in ("tid", "pos", "l_seq", "cig_off", "cigar", "seq_off", "seq", "qual_off", "qual"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


@pytest.fixture(scope="module")
def lib(lib_built):
    return _lib.load()


@pytest.mark.parametrize("name", GOLDENS)
def test_rule_equals_model_reader(lib, golden_dir, name):
    path = os.path.join(golden_dir, name)
    _, _, want, counts = bm.kept_reads(path)
    got, got_counts = batch_by_rule(lib, path)
    assert got_counts == counts
    same_batch(got, want)
    if name == "synth_longcigar.bam":
        assert int(np.diff(got["cig_off"]).max()) == 140000      # the CG:B,I words, not the placeholder's two


def test_rule_filters(lib, golden_dir):
    path = os.path.join(golden_dir, "bbmap.sorted.bam")
    _, _, want, counts = bm.kept_reads(path)
    for kw in ({"min_mapq": 30}, {"flag_filter": 0x714}):
        _, _, w, c = bm.kept_reads(path, **kw)
        assert 0 < c["kept"] < counts["kept"]
        got, got_c = batch_by_rule(lib, path, **kw)
        assert got_c == c
        same_batch(got, w)


def body_of(rec, **kw):
    return synth.encode_record(rec, **kw)[4:]


def test_rule_by_hand(lib):
    plain = SynthRecord("r1", 1, 100, 0x1, [(S, 2), (M, 5)], 7, seq="ACGTNAC")
    b = body_of(plain)
    rc, out = rule(lib, b, 2)
    c_at = 32 + 3
    assert (rc, out) == (TAKEN, [1, 100, 7, 2, c_at, c_at + 8, c_at + 8 + 4])
    assert b[out[5]:out[5] + 4] == bytes([0x12, 0x48, 0xF1, 0x20]) and b[out[6]:out[6] + 7] == bytes([30] * 7)
    # each drop reason: no contig, a filtered flag, MAPQ (encode_record writes 60)
    assert rule(lib, body_of(SynthRecord("u", -1, -1, 0x4, [], 7)), 2)[0] == DROPPED
    for flag in (0x4, 0x100, 0x200, 0x400):
        assert rule(lib, body_of(SynthRecord("f", 0, 5, flag, [(M, 7)], 7)), 2)[0] == DROPPED
    assert rule(lib, body_of(SynthRecord("f", 0, 5, 0x800, [(M, 7)], 7)), 2)[0] == TAKEN
    assert rule(lib, body_of(SynthRecord("f", 0, 5, 0x800, [(M, 7)], 7)), 2, flag_filter=0xF04)[0] == DROPPED
    assert rule(lib, b, 2, min_mapq=60)[0] == TAKEN and rule(lib, b, 2, min_mapq=61)[0] == DROPPED
    # kept, but skipped: no SEQ; no CIGAR; a CIGAR of another query length
    assert rule(lib, body_of(SynthRecord("n", 0, 5, 0, [(M, 7)], 0)), 2)[0] == NO_SEQ
    assert rule(lib, body_of(SynthRecord("n", 0, 5, 0, [], 7)), 2)[0] == BAD_CIGAR
    assert rule(lib, body_of(SynthRecord("n", 0, 5, 0, [(M, 6), (D, 1)], 7)), 2)[0] == BAD_CIGAR
    # the filters come first: a dropped record without SEQ is not counted as no_seq
    assert rule(lib, body_of(SynthRecord("n", 0, 5, 0x400, [(M, 7)], 0)), 2)[0] == DROPPED
    # malformed: tid outside [-1, n_ref), a negative l_seq, a body shorter than its fields say
    assert rule(lib, b, 1)[0] == MALFORMED
    assert rule(lib, struct.pack("<i", -2) + b[4:], 2)[0] == MALFORMED
    assert rule(lib, b[:16] + struct.pack("<i", -1) + b[20:], 2)[0] == MALFORMED
    assert rule(lib, b[:16] + struct.pack("<i", 8) + b[20:], 2)[0] == MALFORMED       # QUAL past the record
    assert rule(lib, b[:12] + struct.pack("<H", 4) + b[14:], 2)[0] == MALFORMED       # CIGAR + SEQ past it
    # (malformed is checked on every record, as the host source checks it, dropped ones included)
    u = body_of(SynthRecord("u", -1, -1, 0x4, [], 7))
    assert rule(lib, u[:16] + struct.pack("<i", 1000) + u[20:], 2)[0] == MALFORMED


def test_rule_placeholder(lib, tmp_path):
    ops = [(M, 3), (I, 1), (M, 2), (D, 4), (M, 1)]
    rec = SynthRecord("cg", 0, 10, 0, ops, 7, seq="ACGTACG")
    tagged = body_of(rec, long_cigar_threshold=2)
    assert struct.unpack_from("<H", tagged, 12)[0] == 2 and b"CGBI" in tagged
    rc, out = rule(lib, tagged, 1)
    assert rc == TAKEN and out[3] == 5 and out[4] == tagged.index(b"CGBI") + 8
    assert np.frombuffer(tagged, "<u4", 5, out[4]).tolist() == [(ln << 4) | op for op, ln in ops]
    # the placeholder without its tag stays the CIGAR (<l_seq>S<n>N has the query length l_seq): as the host source
    bare = SynthRecord("ph", 0, 10, 0, [(S, 7), (N, 11)], 7, seq="ACGTACG")
    rc, out = rule(lib, body_of(bare), 1)
    assert rc == TAKEN and out[3] == 2
    # a tag of another query length makes the record bad_cigar
    short = body_of(SynthRecord("cg", 0, 10, 0, ops[:-1], 6, seq="ACGTAC"), long_cigar_threshold=2)
    short = short[:16] + struct.pack("<i", 6) + short[20:]
    assert rule(lib, short, 1)[0] == TAKEN
    wrong = bytearray(short)
    at = wrong.index(b"CGBI") + 8
    wrong[at:at + 4] = struct.pack("<I", (4 << 4) | M)          # 3M -> 4M: query length 7, l_seq 6
    assert rule(lib, bytes(wrong), 1)[0] == BAD_CIGAR
    # all three through the host source
    from metacov_amd.bases import BaseSource
    path = tmp_path / "ph.bam"
    synth.write_bam(str(path), ["c"], [1000], [rec, bare], long_cigar_threshold=2)
    with BaseSource(str(path)) as src:
        b = {k: v.copy() for k, v in src.next().items()}
        assert np.diff(b["cig_off"]).tolist() == [5, 2] and src.counts()["bad_cigar"] == 0
    got, counts = batch_by_rule(lib, str(path))
    assert counts == {"records": 2, "kept": 2, "no_seq": 0, "bad_cigar": 0}
    same_batch(got, b)


def cut_bodies():
    """Two records for the truncation sweep: a plain one (every cut is
    malformed) and one with a CG:B,I tag behind other tags (a cut inside the
    aux data leaves a whole record whose tag search runs into the cut)."""
    plain = body_of(SynthRecord("plain", 0, 7, 0, [(S, 1), (M, 8)], 9, seq="ACGTACGTA"))
    ops = [(M, 2), (I, 1)] * 3
    tagged = body_of(SynthRecord("tagged", 0, 7, 0, ops, 9, seq="ACGTACGTA"), long_cigar_threshold=2)
    end = tagged.index(b"CGBI")
    aux = b"NMi" + struct.pack("<i", 3) + b"RGZgrp\0" + b"XBBS" + struct.pack("<iHH", 2, 1, 2)
    return plain, tagged[:end] + aux + tagged[end:]


def test_rule_truncated(lib):
    plain, tagged = cut_bodies()
    for k in range(len(plain)):
        assert rule(lib, plain, 1, length=k)[0] == MALFORMED, k
    assert rule(lib, plain, 1)[0] == TAKEN
    payload_end = 32 + 7 + 8 + 5 + 9
    for k in range(len(tagged) + 1):
        rc, out = rule(lib, tagged, 1, length=k)
        assert rc == (MALFORMED if k < payload_end else TAKEN), k
        if rc == TAKEN:      # the tag only when all of it is inside the cut
            assert out[3] == (6 if k == len(tagged) else 2), k
            assert out[4] + 4 * out[3] <= k and out[6] + out[2] <= k


def test_rule_truncated_asan(lib, tmp_path):
    """The same sweep as a stand-alone program built with host
    AddressSanitizer: every cut lives in a heap block of its own size, so a
    read past the cut aborts the program."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    prog = str(tmp_path / "rec_bases_cuts")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address",
                    "-Xarch_host", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "rec_bases_cuts.hip"),
                    "-o", prog], check=True, capture_output=True)
    for body in cut_bodies():
        rec = tmp_path / "rec.bin"
        rec.write_bytes(body)
        r = subprocess.run([prog, str(rec), "1"], capture_output=True, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.split("\n")[:-1]
        assert len(lines) == len(body) + 1
        for k, line in enumerate(lines):
            rc, out = rule(lib, body, 1, length=k)
            assert int(line.split()[0]) == rc, k
            if rc == TAKEN:
                assert int(line.split()[1]) == out[3], k


def test_abi_table_has_bases_decode():
    for name in ("mc_bam_gpu_open_bases", "mc_bam_gpu_bases_device", "mc_bam_gpu_bases_copy",
                 "mc_bam_gpu_bases_counts", "mc_bases_add_batch_device", "mc_bam_rec_bases_host"):
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["mc_bases_add_batch_device"]) == 14
    assert len(_lib.SIGNATURES["mc_bam_gpu_bases_device"]) == 14


def test_cli_decode_option(golden_dir):
    from metacov_amd.cli import main
    bam = os.path.join(golden_dir, "synth_exp.bam")
    r = CliRunner().invoke(main, ["bases", "-b", bam, "--decode", "cpu"])
    assert r.exit_code == 2 and "--decode" in r.output
    r = CliRunner().invoke(main, ["bases", "--help"])
    assert r.exit_code == 0 and "--decode" in r.output and "host" in r.output and "gpu" in r.output


def test_python_decode_argument(golden_dir):
    from metacov_amd import bases as mb
    with pytest.raises(ValueError, match="decode"):
        mb.count_coverage(os.path.join(golden_dir, "synth_exp.bam"), "x", decode="cpu")
    assert hasattr(mb, "GpuBaseSource") and hasattr(mb.BaseCounter, "add_device")
