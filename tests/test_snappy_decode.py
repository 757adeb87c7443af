"""The Snappy raw decoders byte for byte against pyarrow's bundled Snappy: the host form
(csrc/snappy_host.h) on the CPU, every kernel variant of csrc/snappy_decode.hip on the GPU.

All streams of a test go into one chunk table: one call of the host form, one launch per kernel
variant.  Every stream lies at each of the 16 byte phases of a 16-byte granule in the source buffer
and (through a permutation of the phases) in the destination buffer; a destination has exactly its
capacity and 32 guard bytes on both sides, and every byte outside the destinations must be unchanged
afterwards."""
import os
import shutil
import subprocess

import numpy as np
import pyarrow as pa
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, FILL = 32, 0xA5
CODEC = pa.Codec("snappy")
VARIANTS = [0, 1]


def _lib():
    from alluxio_amd.ops.native import lib
    return lib()


# ---- a small stream builder -----------------------------------------------------------------------------
def _preamble(v: int) -> bytes:
    out = bytearray()
    while v >= 128:
        out.append(128 | (v & 127))
        v >>= 7
    out.append(v)
    return bytes(out)


class Builder:
    """Elements (without the preamble) and the bytes they give."""

    def __init__(self):
        self.body, self.out = bytearray(), bytearray()

    def literal(self, data: bytes, len_bytes: int = 0, apply: bool = True):
        m = len(data) - 1
        if len_bytes == 0 and m < 60:
            self.body.append(m << 2)
        else:
            len_bytes = len_bytes or (1 if m < 256 else 2 if m < 65536 else 3)
            assert m < 256 ** len_bytes
            self.body.append((59 + len_bytes) << 2)
            self.body += m.to_bytes(len_bytes, "little")
        self.body += data
        if apply:
            self.out += data
        return self

    def copy(self, kind: int, length: int, offset: int, apply: bool = True):
        if kind == 1:
            assert 4 <= length <= 11 and offset < 2048
            self.body += bytes([1 | ((length - 4) << 2) | ((offset >> 8) << 5), offset & 255])
        else:
            assert 1 <= length <= 64
            self.body += bytes([kind | ((length - 1) << 2)]) + offset.to_bytes(2 if kind == 2 else 4, "little")
        if apply:
            op = len(self.out)
            for i in range(length):
                self.out.append(self.out[op - offset + i % offset])
        return self

    def stream(self, preamble=None) -> bytes:
        return _preamble(len(self.out) if preamble is None else preamble) + bytes(self.body)


def _noise(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _text(n: int, seed: int = 1) -> bytes:
    rng = np.random.default_rng(seed)
    words = [b"alluxio", b"page", b"cache", b"tier", b"block", b"worker", b"master", b"parquet", b"the", b"quick", b"fox"]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, len(words)))] + (b"\n" if rng.integers(0, 9) == 0 else b" ")
    return bytes(out[:n])


def _compressed(data: bytes):
    z = CODEC.compress(data, asbytes=True)
    return z, data


def _built(b: Builder):
    """A hand-built stream, checked against pyarrow's decoder."""
    z, want = b.stream(), bytes(b.out)
    assert CODEC.decompress(z, decompressed_size=len(want), asbytes=True) == want
    return z, want


def _sequence(b: Builder):
    """A fixed run of every kind of element behind whatever b holds (at least 70 bytes)."""
    b.copy(1, 4, 3).literal(b"xy").copy(2, 64, 1).copy(1, 11, 2047 if len(b.out) >= 2047 else 7)
    b.copy(3, 33, len(b.out)).literal(_noise(61, 5), 1).copy(2, 1, 70).copy(2, 64, 63).literal(b"q", 2)
    b.copy(3, 64, 2).literal(_noise(300, 6)).copy(2, 17, 300).copy(1, 5, 1).literal(_noise(7, 7), 4).copy(2, 64, 7)
    return b


_CACHE = {}


def _sizes():
    return dict(_lib().snappy_decode_sizes())


def _compressor_streams():
    if "compressor" not in _CACHE:
        s = [(b"\x00", b""), _compressed(b"x")]
        assert CODEC.compress(b"", asbytes=True) == b"\x00"
        s += [_compressed(_noise(n, n)) for n in (59, 60, 61, 63, 64, 65)]
        s.append(_compressed(_text(300_000)))
        s.append(_compressed(np.arange(50_000, dtype=np.int64).tobytes()))          # ~100,000 short elements
        s.append(_compressed(_noise(200_000, 3)))                                   # 64 KiB literals
        s.append(_compressed(bytes(1024 * 1024 + 17)))                              # 64-byte copies at offset 1
        _CACHE["compressor"] = s
    return _CACHE["compressor"]


def _exact(n: int, head: bool) -> Builder:
    """A stream of exactly n bytes: (with head) a few elements of every kind, then one literal."""
    b = Builder()
    if head:
        b.literal(_noise(20, n)).copy(1, 4, 3).copy(2, 64, 1).copy(3, 10, 20).copy(1, 11, 90)
    for fill in range(n, 0, -1):
        if len(_preamble(len(b.out) + fill)) + len(b.body) + 3 + fill == n:
            return b.literal(_noise(fill, n + 1), 2)
    raise AssertionError(n)


def _boundary_streams():
    """For each buffer size of the kernels, streams whose uncompressed or compressed length is one
    below, equal to and one above it."""
    if "boundary" not in _CACHE:
        s = []
        for size in sorted(set(v for k, v in _sizes().items() if k != "default_variant")):
            for n in (size - 1, size, size + 1):
                s.append(_compressed(_text(n, n)))
                s.append(_compressed(_noise(n, n)))
                for head in (False, True):                     # compressed length n
                    s.append(_built(_exact(n, head)))
        _CACHE["boundary"] = s
    return _CACHE["boundary"]


def _hand_streams():
    if "hand" not in _CACHE:
        s = [_built(Builder().literal(b"abcdefghijklmnop").copy(1, 7, 5).copy(2, 33, 16).copy(3, 64, 23).literal(b"z"))]
        for len_bytes in (1, 2, 3, 4):                                              # tags 60 to 63
            n = 70_000 if len_bytes == 3 else 60 + len_bytes
            s.append(_built(Builder().literal(_noise(n, n), len_bytes).copy(2, 10, 3)))
        far = Builder().literal(_noise(70_000, 9), 3).copy(3, 64, 9).copy(3, 50, 66_000)
        s.append(_built(far.copy(3, 64, len(far.out)).copy(2, 1, 1)))               # kind 3 near and far, to byte 0, length 1
        for off in (1, 2, 3, 7, 63):                                                # overlapping copies
            s.append(_built(Builder().literal(_noise(off, off)).copy(2, 64, off).copy(2, 64, off).copy(3, 64, off)))
        s.append(_built(Builder().literal(b"abcd").copy(2, 4, 4)))                  # the offset equals the bytes produced
        s.append(_built(Builder().literal(b"a").copy(2, 1, 1)))
        for prefix in range(0, 81):                                                 # every phase of a 64-byte window
            b = Builder()
            if prefix:
                b.literal(_noise(prefix, prefix))
            s.append(_built(_sequence(b.literal(_noise(90, 90 + prefix), 2 if prefix % 2 else 0))))
        # a long run of short elements behind a long literal: stage and ring boundaries inside the run
        b = Builder().literal(_noise(5000, 11))
        for i in range(1500):
            b.copy(1, 4 + i % 8, 1 + (i * 37) % 2040).literal(_noise(1 + i % 5, i))
            if i % 100 == 0:
                b.copy(3, 64, 4500 + i)
        s.append(_built(b))
        _CACHE["hand"] = s
    return _CACHE["hand"]


def _malformed_streams():
    """(stream, capacity): each refused by pyarrow's decoder too."""
    if "malformed" not in _CACHE:
        lit8 = Builder().literal(b"abcdefgh")
        s = [(Builder().literal(b"abcd").copy(2, 4, 0, apply=False).stream(8), 8),          # offset 0
             (Builder().literal(b"abcd").copy(2, 4, 5, apply=False).stream(8), 8),          # one past the produced bytes
             (Builder().literal(b"abcd").copy(1, 4, 5, apply=False).stream(8), 8),
             (Builder().literal(b"abcd").copy(3, 4, 70_000, apply=False).stream(8), 8),
             (Builder().literal(b"abcd").copy(2, 5, 4, apply=False).stream(8), 8),          # a copy one byte past cap
             (Builder().literal(b"abcde").stream(4), 4),                                    # a literal one byte past cap
             (lit8.stream()[:-1], 8),                                                       # a literal cut short
             (Builder().literal(_noise(3000, 1), 2).stream()[:-1], 3000),
             (lit8.stream(9), 9),                                                           # one byte short of the preamble
             (lit8.stream(9), 8),                                                           # the preamble is not cap
             (lit8.stream(7), 7),
             (b"\x88\x80\x80\x80\x80\x00" + bytes(lit8.body), 8)]                           # a 6-byte preamble
        for kind in (1, 2, 3):                                                              # a header cut short
            s.append((Builder().literal(b"abcdefgh").copy(kind, 4, 2, apply=False).stream(12)[:-1], 12))
        s.append((_preamble(300) + bytes([61 << 2, 0x2B]), 300))                            # ... a literal's length bytes
        # behind 200 good elements, so that the error lies deep in the stream
        deep = Builder().literal(_noise(100, 2))
        for i in range(200):
            deep.copy(1, 4 + i % 8, 1 + i % 90).literal(_noise(1 + i % 3, i))
        s.append((_preamble(len(deep.out) + 4) + bytes(deep.body) + bytes([2 | (3 << 2), 0, 0]), len(deep.out) + 4))
        for z, cap in s:
            with pytest.raises(Exception):
                CODEC.decompress(z, decompressed_size=cap, asbytes=True)
        _CACHE["malformed"] = s
    return _CACHE["malformed"]


# ---- one table, one call -----------------------------------------------------------------------------------
def _run(streams, device, phases=range(16)):
    """streams: (stream, expected bytes) or, for a malformed one, (stream, capacity).  device:
    "host" for the host form, else a torch device for the current kernel variant."""
    entries, so, do = [], 0, 0
    for i, (z, want) in enumerate(streams):
        cap = want if isinstance(want, int) else len(want)
        for p in phases:
            so = (so + 15) // 16 * 16 + p
            do = (do + 15) // 16 * 16 + GUARD + (p * 7 + 3 + i) % 16
            entries.append((so, do, z, cap, want))
            so += len(z)
            do += cap + GUARD
    src = np.full(so + 16, 0x5A, dtype=np.uint8)
    dst = np.full(do + 16, FILL, dtype=np.uint8)
    owned = np.zeros(len(dst), dtype=bool)
    for s0, d0, z, cap, _w in entries:
        src[s0:s0 + len(z)] = np.frombuffer(z, dtype=np.uint8)
        owned[d0:d0 + cap] = True
    C = _lib()
    if device == "host":
        sizes = C.snappy_host([(src.ctypes.data + s0, dst.ctypes.data + d0, len(z), cap) for s0, d0, z, cap, _w in entries])
    else:
        import torch
        d_src, d_dst = torch.from_numpy(src).to(device), torch.from_numpy(dst).to(device)
        sizes = C.snappy_device([(d_src.data_ptr() + s0, d_dst.data_ptr() + d0, len(z), cap)
                                 for s0, d0, z, cap, _w in entries], torch.cuda.current_stream().cuda_stream)
        dst = d_dst.cpu().numpy()
    assert (dst[~owned] == FILL).all(), "bytes outside the destinations were written"
    wrong = []
    for k, ((s0, d0, z, cap, want), size) in enumerate(zip(entries, sizes)):
        if isinstance(want, int):
            if size >= 0:
                wrong.append((k // len(phases), "accepted", size))
        elif size != cap or dst[d0:d0 + cap].tobytes() != want:
            wrong.append((k // len(phases), k % len(phases), size, cap))
    assert not wrong, wrong[:10]
    return sizes


# ---- CPU: the host form -----------------------------------------------------------------------------------
def test_snappy_host_compressor_streams():
    _run(_compressor_streams(), "host")


def test_snappy_host_boundary_streams():
    _run(_boundary_streams(), "host")


def test_snappy_host_hand_built_streams():
    _run(_hand_streams(), "host")


def test_snappy_host_malformed_streams():
    good = _hand_streams()[0]
    sizes = _run(_malformed_streams() + [good], "host")
    assert sizes[-1] == len(good[1])
    C = _lib()
    with pytest.raises(Exception, match="malformed snappy"):
        C.snappy_decompress(_malformed_streams()[0][0], 8)
    assert C.snappy_decompress(good[0], len(good[1])) == good[1]


def test_snappy_host_check_program(tmp_path):
    """tools/snappy_host_check.cpp builds with the command in its header and prints ok."""
    from alluxio_amd.ops.build import ROCM
    cxx = shutil.which("clang++") or os.path.join(ROCM, "lib", "llvm", "bin", "clang++")
    exe = str(tmp_path / "snappy_host_check")
    header = open(os.path.join(ROOT, "tools", "snappy_host_check.cpp")).read().split("#include")[0]
    flags = "-std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined"
    sources = "tools/snappy_host_check.cpp"
    assert flags in header and "-Ialluxio_amd/csrc " + sources in header
    subprocess.run([cxx, *flags.split(), "-Ialluxio_amd/csrc", *sources.split(), "-o", exe], cwd=ROOT, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---- GPU: every kernel variant ----------------------------------------------------------------------------
@pytest.fixture(params=[pytest.param(v, id=f"v{v}") for v in VARIANTS])
def variant(request, gpu):
    C = _lib()
    C.set_snappy_decode_variant(request.param)
    yield request.param
    C.set_snappy_decode_variant(-1)


@pytest.mark.gpu
def test_snappy_compressor_streams(variant):
    _run(_compressor_streams(), "cuda")


@pytest.mark.gpu
def test_snappy_boundary_streams(variant):
    _run(_boundary_streams(), "cuda")


@pytest.mark.gpu
def test_snappy_hand_built_streams(variant):
    _run(_hand_streams(), "cuda")


@pytest.mark.gpu
def test_snappy_malformed_streams(variant):
    """The bounds checks: every malformed stream gives a negative size and leaves the guards alone,
    and a well-formed stream of the same launch decodes."""
    good = _hand_streams()[0]
    sizes = _run(_malformed_streams() + [good], "cuda")
    assert sizes[-1] == len(good[1])


@pytest.mark.gpu
def test_snappy_default_variant(gpu):
    """Variant -1 is the default of the profile, and an unknown variant is an error, not a fallback."""
    C = _lib()
    C.set_snappy_decode_variant(-1)
    _run(_hand_streams()[:3], "cuda", phases=[5])
    C.set_snappy_decode_variant(7)
    try:
        with pytest.raises(Exception):
            _run(_hand_streams()[:1], "cuda", phases=[0])
    finally:
        C.set_snappy_decode_variant(-1)
