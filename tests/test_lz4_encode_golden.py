"""The LZ4 encoders give the bytes they gave before: size and SHA-256 of every block, for fixed
inputs, against tests/golden/lz4_encode_blocks.json.  The other tests compare what blocks decode
to; a change to the parse that is meant to leave the output alone is held to this one.

The chunk encoder (csrc/lz4_encode.hip, every ``set_lz4_encode_variant``) runs once per variant
over every length x content below, sources and destinations at odd addresses, plus one chunk whose
capacity is half its length.  71 chunks in one call: variant 4 takes the segmented path with S = 8,
variant 3 with S = 4.  The page encoder's blocks are those that ``_run_direct`` of
test_parquet_write_lz4.py builds, at its three segment sizes.

The fixture was recorded twice, in separate processes, from the tree before the encoders moved to
a file of their own; the two recordings agreed."""
import hashlib
import json
import os

import numpy as np
import pytest
from test_parquet_write_lz4 import _content, _run_direct

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz4_encode_blocks.json")
# the block end rules (0..13), one probe batch (64, 65), each threshold of the segment count (4 KiB
# steps up to 8 segments), the longest chunk
LENGTHS = [0, 1, 12, 13, 64, 65, 4095, 4096, 8191, 8192, 16383, 32768, 65535, 65536]
KINDS = ["constant", "period3", "words", "csv", "random"]
VARIANTS = [0, 1, 2, 3, 4]
SEGMENTS = [16 * 1024, 32 * 1024, 60 * 1024]
HALF = ("random", 65536)                                # encoded again into half its length: -1


def _digest(block: bytes):
    return [len(block), hashlib.sha256(block).hexdigest()]


def _odd(buf: bytearray, fill: int):
    """Pad buf to an odd length (an odd address in a buffer that starts at an even one)."""
    buf += bytes([fill]) * (1 if len(buf) % 2 == 0 else 2)
    return len(buf)


def chunk_blocks(device):
    """{variant: {"kind/length": block}} from one call of every chunk per variant."""
    import torch
    from alluxio_amd.ops.native import lib
    C = lib()
    raws = {(kind, n): _content(kind, n) for n in LENGTHS for kind in KINDS}
    src, places, at, caps = bytearray(), [], [], []
    out_bytes = bytearray()
    for raw in list(raws.values()) + [raws[HALF]]:
        places.append(_odd(src, 0xEE))
        src += raw
        caps.append(C.lz4_compress_bound(len(raw)))
        at.append(_odd(out_bytes, 0xAA))
        out_bytes += b"\xAA" * caps[-1]
    caps[-1] = len(raws[HALF]) // 2
    out_bytes += b"\xAA"
    t_src = torch.from_numpy(np.frombuffer(bytes(src), dtype=np.uint8).copy()).to(device)
    assert t_src.data_ptr() % 2 == 0
    lens = [len(r) for r in raws.values()] + [len(raws[HALF])]
    got = {}
    try:
        for v in VARIANTS:
            C.set_lz4_encode_variant(v)
            out = torch.from_numpy(np.frombuffer(bytes(out_bytes), dtype=np.uint8).copy()).to(device)
            assert out.data_ptr() % 2 == 0
            sizes = C.lz4_device([(t_src.data_ptr() + p, out.data_ptr() + a, n, k)
                                  for p, a, n, k in zip(places, at, lens, caps)], True, 0)
            assert sizes[-1] == -1, (v, sizes[-1])       # half the capacity: refused in every variant
            blob = out.cpu().numpy().tobytes()
            blocks = {}
            for (key, raw), a, k, size in zip(raws.items(), at, caps, sizes):
                assert 1 <= size <= k, (v, key, size)
                block = blob[a:a + size]
                assert C.lz4_decompress(block, len(raw)) == raw, (v, key)
                assert blob[a + k:a + k + 1] == b"\xAA", (v, key)      # nothing behind its capacity
                blocks[f"{key[0]}/{key[1]}"] = block
            got[str(v)] = blocks
    finally:
        C.set_lz4_encode_variant(4)
    return got


def page_blocks(device):
    """{segment: {"kind/length": block}}; _run_direct has decoded each block to its body."""
    return {str(seg): {f"{k[0]}/{k[1]}": b for k, b in _run_direct(device, seg).items()} for seg in SEGMENTS}


def digests(blocks):
    return {group: {key: _digest(b) for key, b in items.items()} for group, items in blocks.items()}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _compare(got, want):
    assert sorted(got) == sorted(want)
    for group in want:
        assert sorted(got[group]) == sorted(want[group]), group
        moved = {key: (got[group][key], want[group][key]) for key in want[group] if got[group][key] != want[group][key]}
        assert not moved, (group, moved)


def test_chunk_blocks_unchanged(gpu, golden):
    _compare(digests(chunk_blocks(gpu)), golden["chunk"])


def test_page_blocks_unchanged(gpu, golden):
    _compare(digests(page_blocks("cuda")), golden["page"])
