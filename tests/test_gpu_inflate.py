"""gz_inflate_kernel (csrc/bam_gpu.hip, lane code csrc/inflate.h) byte for
byte against zlib.

The host instantiation of inflate.h is tested in test_gpu_decode.py
(mc_gz_inflate_host: one lane, plain arrays, no wave vote).  Here the kernel
itself runs, through mc_gz_inflate_device, on waves the product's BAMs never
form: lanes holding stored, fixed, dynamic, RLE and Huffman-only payloads of
0 - 65536 bytes at once, payloads of several deflate blocks, every source
alignment, lanes that leave at once, lanes taking several blocks in turn (the
grid-stride loop) and bad payloads among good ones.  The output buffer is
filled with 0xAA before the launch and comes back whole, so every byte
outside a block's own range is checked too.  Expected bytes are the original
data; every payload is first checked against zlib.decompress on the CPU.
"""
import zlib

import numpy as np
import pytest

from metacov_amd._lib import MC_E_INVALID, MetacovError, check
from tests.test_gpu_decode import _flushed, _inflate_host, _rare_matches, _raw_deflate

pytestmark = pytest.mark.gpu

GUARD = 48          # untouched bytes between output ranges in the guarded layout
TAIL = 64           # untouched bytes after the last output range, both layouts
FILL = 0xAA
SIZES = [0, 1, 2, 3, 15, 16, 17, 257, 4096, 65279, 65280, 65536]
EMPTY = b"\x03\x00"  # the BGZF EOF block's payload: a final fixed block holding only the end code


# ---------------------------------------------------------------- payloads

def _acgtn(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), n, p=[.3, .2, .2, .29, .01]))


def _random(rng, n):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


def _xs(rng, n):
    return b"x" * n


def _ramp(rng, n):
    return (bytes(range(256)) * (n // 256 + 1))[:n]


def _rare(rng, n):
    return _rare_matches(int(rng.integers(1 << 30)), n)


def _sync_then_finish(data):
    """Everything, a sync flush, then finish: an empty stored block before an
    empty final block."""
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    return c.compress(data) + c.flush(zlib.Z_SYNC_FLUSH) + c.flush()


F, R, H = zlib.Z_FIXED, zlib.Z_RLE, zlib.Z_HUFFMAN_ONLY

# name -> (data maker, compressor); every kind takes any size
KINDS = [
    ("stored", _acgtn, lambda d: _raw_deflate(d, 0)),
    ("fixed", _acgtn, lambda d: _raw_deflate(d, 6, F)),
    ("dynamic1", _acgtn, lambda d: _raw_deflate(d, 1)),
    ("dynamic6-rare", _rare, lambda d: _raw_deflate(d, 6)),
    ("dynamic9", _acgtn, lambda d: _raw_deflate(d, 9)),
    ("rle-ramp", _ramp, lambda d: _raw_deflate(d, 6, R)),
    ("rle-x", _xs, lambda d: _raw_deflate(d, 1, R)),
    ("huffman-only", _acgtn, lambda d: _raw_deflate(d, 6, H)),
    ("huffman-only-random", _random, lambda d: _raw_deflate(d, 9, H)),
    ("random6", _random, lambda d: _raw_deflate(d, 6)),          # zlib falls back to stored blocks
    ("fixed-random", _random, lambda d: _raw_deflate(d, 1, F)),  # 9-bit literals
    ("ramp9", _ramp, lambda d: _raw_deflate(d, 9)),              # length 258 at distance 256
    ("x9", _xs, lambda d: _raw_deflate(d, 9)),                   # overlapping copies at distance 1
    ("sync-flush6", _acgtn, lambda d: _flushed(d, 6, zlib.Z_SYNC_FLUSH)),
    ("full-flush1-rare", _rare, lambda d: _flushed(d, 1, zlib.Z_FULL_FLUSH)),
    ("sync-flush-fixed", _ramp, lambda d: _flushed(d, 9, zlib.Z_SYNC_FLUSH, strategy=F)),
    ("sync-then-finish", _acgtn, _sync_then_finish),
]
# kinds of one size: (name, size)
SPECIALS = [("stored-65536", 65536), ("far-match", 32768 + 258), ("eof", 0)]


class _BitWriter:
    """Deflate bit order: fields from the low bit of each byte up; Huffman
    codes most significant bit first (RFC 1951 §3.1.1)."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, n):
        self.bits(int(format(v, "0%db" % n)[::-1], 2), n)

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def _far_match(rng):
    """A hand-written fixed-Huffman block: 32768 literals, then a match of
    length 258 at distance 32768, the format's largest (zlib's own deflate
    never emits one above 32506)."""
    lit = _random(rng, 32768)
    w = _BitWriter()
    w.bits(1, 1)        # BFINAL
    w.bits(1, 2)        # BTYPE 01: fixed codes
    for v in lit:
        if v < 144:
            w.code(0x30 + v, 8)
        else:
            w.code(0x190 + v - 144, 9)
    w.code(0xC0 + 285 - 280, 8)     # length symbol 285: 258, no extra bits
    w.code(29, 5)                   # distance symbol 29: 24577 + 13 extra bits
    w.bits(32768 - 24577, 13)
    w.code(0, 7)                    # end of block (symbol 256)
    return lit + lit[:258], w.done()


def _special(name, rng):
    if name == "stored-65536":      # level 0 at 65536 bytes: two stored blocks (65535 + 1)
        data = _acgtn(rng, 65536)
        return data, _raw_deflate(data, 0)
    if name == "far-match":
        return _far_match(rng)
    return b"", EMPTY


class Block:
    def __init__(self, kind, data, payload):
        # the reference alone satisfies the test: zlib gives the original bytes
        assert zlib.decompress(payload, -15) == data, kind
        self.kind, self.data, self.payload = kind, data, payload


def _wave(w):
    """32 blocks (one wave's) holding every kind and every size class; the
    kinds rotate by 5 per wave, so blocks b and b + 32 differ in kind."""
    rng = np.random.default_rng(1000 + w)
    names = [k[0] for k in KINDS] + [s[0] for s in SPECIALS]
    out, g = [], 0
    for j in range(32):
        k = (j + 5 * w) % len(names)
        if k < len(KINDS):
            name, make, comp = KINDS[k]
            n = SIZES[(g + 7 * w) % len(SIZES)]
            g += 1
            data = make(rng, n)
            out.append(Block("%s/%d" % (name, n), data, comp(data)))
        else:
            data, payload = _special(names[k], rng)
            out.append(Block(names[k], data, payload))
    return out


@pytest.fixture(scope="module")
def zoo(lib_built):
    blocks = [b for w in range(6) for b in _wave(w)]
    assert len(blocks) == 192
    n_kinds = len(KINDS) + len(SPECIALS)
    for w in range(6):
        wave = blocks[32 * w:32 * w + 32]
        assert len({b.kind.split("/")[0] for b in wave}) == n_kinds
        assert {len(b.data) for b in wave} >= set(SIZES)
    for a, b in zip(blocks, blocks[32:]):
        assert a.kind.split("/")[0] != b.kind.split("/")[0]
    far = next(b for b in blocks if b.kind == "far-match")
    rc, got = _inflate_host(far.payload, len(far.data))     # the host lane code takes the hand-written stream
    assert rc == 0 and got == far.data
    return blocks


# ---------------------------------------------------------------- the hook

def _lib():
    from metacov_amd import _lib as L
    return L.load()


def _pack(blocks):
    """Payloads in one buffer, block b's at an offset equal to b modulo 16
    (gaps of 0 - 15 bytes of 0xFF), so all 16 source alignments occur."""
    comp, cdata = bytearray(), []
    for b, blk in enumerate(blocks):
        comp += b"\xff" * ((b - len(comp)) % 16)
        cdata.append(len(comp))
        comp += blk.payload
    assert len(blocks) < 16 or {c % 16 for c in cdata} == set(range(16))
    return bytes(comp), np.array(cdata, np.int64)


def _launch(comp, cdata, clen, out_off, isize, out_bytes, max_lanes=0, out=None):
    lib = _lib()
    cdata, out_off = np.ascontiguousarray(cdata, np.int64), np.ascontiguousarray(out_off, np.int64)
    clen, isize = np.ascontiguousarray(clen, np.int32), np.ascontiguousarray(isize, np.int32)
    out = np.full(out_bytes, 0x55, np.uint8) if out is None else out
    status = np.full(len(cdata), -7, np.int32)
    check(lib.mc_gz_inflate_device(0, len(cdata), comp, len(comp), cdata.ctypes.data, clen.ctypes.data,
                                   out_off.ctypes.data, isize.ctypes.data, out.ctypes.data, out_bytes,
                                   max_lanes, status.ctypes.data), lib)
    return status, out


def _run(blocks, guard, max_lanes=0, isize=None):
    """The blocks through the kernel: (status, out, out_off).  isize: sizes
    other than the data's (bad blocks)."""
    comp, cdata = _pack(blocks)
    isize = np.array([len(b.data) for b in blocks] if isize is None else isize, np.int64)
    out_off = np.concatenate([[0], np.cumsum(isize + guard)[:-1]]).astype(np.int64)
    out_bytes = int(out_off[-1] + isize[-1]) + TAIL
    status, out = _launch(comp, cdata, [len(b.payload) for b in blocks], out_off, isize, out_bytes, max_lanes)
    return status, out, out_off


def _check(blocks, status, out, out_off, isize=None, bad=()):
    """Every good block: status 0 and exactly its bytes.  Every byte outside
    the blocks' ranges (guards, the tail): still the fill."""
    covered = np.zeros(len(out), bool)
    for i, (b, o) in enumerate(zip(blocks, out_off)):
        n = len(b.data) if isize is None else int(isize[i])
        covered[o:o + n] = True
        if i in bad:
            assert status[i] != 0, (i, b.kind)
            continue
        assert status[i] == 0, (i, b.kind, int(status[i]))
        got = out[o:o + n].tobytes()
        if got != b.data:
            at = next(k for k in range(n) if got[k] != b.data[k])
            raise AssertionError("block %d (%s): byte %d of %d is %#x, not %#x"
                                 % (i, b.kind, at, n, got[at], b.data[at]))
    stray = np.flatnonzero(~covered & (out != FILL))
    assert stray.size == 0, "bytes outside every output range were written, first at %d" % stray[0]
    assert (~covered).sum() >= TAIL


_runs = {}


def _zoo_run(zoo, guard, max_lanes):
    key = (guard, max_lanes)
    if key not in _runs:
        _runs[key] = _run(zoo, guard, max_lanes)
    return _runs[key]


def _lanes_per_wave():
    """The smallest max_lanes the hook takes (it refuses anything but a
    multiple of the kernel's lanes per wave before it touches the device)."""
    lib = _lib()
    for lanes in (8, 16, 32, 64):
        if lib.mc_gz_inflate_device(0, 0, None, 0, None, None, None, None, None, 0, lanes, None) == 0:
            return lanes
    raise AssertionError("the header promises that max_lanes = 64 is accepted")


# ---------------------------------------------------------------- tests

@pytest.mark.parametrize("guard", [0, GUARD])
def test_device_matches_zlib_mixed_waves(zoo, guard):
    """192 blocks, every wave of 32 holding every payload kind and size
    class, outputs contiguous (the product's layout) and 48 bytes apart."""
    status, out, out_off = _zoo_run(zoo, guard, 0)
    _check(zoo, status, out, out_off)


@pytest.mark.parametrize("waves", [1, 2])
def test_device_grid_stride_few_lanes(zoo, waves):
    """The same blocks on one and two waves: every lane inflates 6 (3)
    blocks in turn, starting each while its mates are inside theirs."""
    lanes = _lanes_per_wave() * waves
    assert lanes < len(zoo)
    for guard in (0, GUARD):
        status, out, out_off = _zoo_run(zoo, guard, lanes)
        _check(zoo, status, out, out_off)
        ref_status, ref_out, _ = _zoo_run(zoo, guard, 0)
        assert np.array_equal(status, ref_status) and np.array_equal(out, ref_out)


def test_device_early_exit_lanes(lib_built):
    """One wave: lanes 0, 5 and 31 hold empty blocks and lanes 1 and 30
    one-byte blocks, leaving while the other 27 vote through 65280-byte
    level-9 blocks."""
    rng = np.random.default_rng(7)
    blocks = []
    for j in range(32):
        if j in (0, 5, 31):
            blocks.append(Block("eof", b"", EMPTY))
        elif j in (1, 30):
            data = bytes([65 + j])
            blocks.append(Block("one-byte", data, _raw_deflate(data, 9)))
        else:
            data = _acgtn(rng, 65280)
            blocks.append(Block("dynamic9/65280", data, _raw_deflate(data, 9)))
    for guard in (0, GUARD):
        status, out, out_off = _run(blocks, guard)
        _check(blocks, status, out, out_off)


def test_device_error_isolated(zoo):
    """A bad payload in lane 16 of a wave of good ones: its status alone is
    non-zero, the other 31 blocks are exact, and nothing is written outside
    the output ranges, the 48 bytes after the bad block's own included."""
    x = b"x" * 1000
    good = _raw_deflate(_acgtn(np.random.default_rng(3), 40_000), 6)
    nlen = b"\x01" + (100).to_bytes(2, "little") + (100).to_bytes(2, "little") + b"s" * 100
    bads = [("block-type-3", b"\x07\x00\x00\x00", 100),
            ("stored-wrong-nlen", nlen, 100),
            ("isize-one-too-small", _raw_deflate(x, 6), 999),
            ("isize-one-too-large", _raw_deflate(x, 6), 1001),
            ("cut-in-half", good[:len(good) // 2], 40_000)]
    blocks, isize, bad = [], [], []
    for w, (name, payload, n) in enumerate(bads):
        rc, _ = _inflate_host(payload, n)       # the host lane code refuses it first
        assert rc != 0, name
        wave = list(zoo[32 * w:32 * w + 32])
        sizes = [len(b.data) for b in wave]
        blk = Block.__new__(Block)
        blk.kind, blk.data, blk.payload = name, b"", payload
        wave[16], sizes[16] = blk, n
        bad.append(32 * w + 16)
        blocks += wave
        isize += sizes
    status, out, out_off = _run(blocks, GUARD, isize=isize)
    _check(blocks, status, out, out_off, isize=isize, bad=set(bad))


def test_hook_argument_errors(lib_built):
    """Overlapping outputs, a payload past the compressed bytes and a bad
    max_lanes are refused before anything is launched or copied."""
    comp = _raw_deflate(b"x" * 100, 6) * 2
    h = len(comp) // 2
    ok = dict(comp=comp, cdata=[0, h], clen=[h, h], out_off=[0, 100], isize=[100, 100], out_bytes=200)
    status, out = _launch(**ok)
    assert not status.any() and out.tobytes() == b"x" * 200
    for change in (dict(out_off=[0, 99]), dict(out_off=[50, 0], isize=[100, 100]), dict(clen=[h, h + 1]),
                   dict(cdata=[0, -1]), dict(out_off=[0, 101]), dict(max_lanes=7), dict(max_lanes=-64)):
        out = np.full(200, 0x55, np.uint8)
        with pytest.raises(MetacovError) as e:
            _launch(**dict(ok, out=out, **change))
        assert e.value.code == MC_E_INVALID and (out == 0x55).all(), change
