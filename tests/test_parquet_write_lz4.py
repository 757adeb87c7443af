"""write_parquet_columns / ParquetWriter with compression="lz4_raw": every page body as one LZ4
block made where the columns lie (csrc/lz4_block_host.h; the page kernels of csrc/lz4_encode.hip).
Blocks are compared here by what they decode to and by their sizes: the device parse has a benign
race in its hash table, and the host parse is another one.  (The bytes the device has given so far
are held by test_lz4_encode_golden.py.)  The CPU variants run the host form on a
DRAM-tier cluster, the ``gpu`` ones the kernels on the HBM tier."""
import io
import os
import shutil
import subprocess

import numpy as np
import pyarrow.parquet as pq
import pytest
from test_parquet_columns import _cluster
from test_parquet_write import ROOT, _arrow, _check, _col, _launches, _read, _same, _write_spec

from alluxio_amd.models import FieldColumns, ParquetWriter, parquet_metadata, read_parquet_columns, write_parquet_columns
from alluxio_amd.models.parquet import lz4_block_tables

S = 32 * 1024                                           # the segment
SIZES = [0, 1, 12, 13, 4095, S - 1, S, S + 1, 2 * S + 1, 10 * S + 7]
WORDS = ["the", "quick", "brown", "fox", "jumps", "over", "lazy", "dog", "alluxio", "page", "cache", "tier", "block",
         "worker", "master", "parquet"]
CONTENTS = ["constant", "random", "random-then-repetitive", "repetitive-then-random", "period3", "words", "csv"]


def _content(kind: str, n: int, seed: int = 0, ascii_only: bool = False) -> bytes:
    """n bytes of one of the issue's contents from a seeded generator."""
    rng = np.random.default_rng(seed * 1000 + n)
    noise = lambda k: rng.integers(0x20 if ascii_only else 0, 0x7F if ascii_only else 256, k, dtype=np.uint8).tobytes()
    rep = lambda k, at=0: bytes(97 + (at + i) % 7 for i in range(k))
    if kind == "constant":
        return b"a" * n
    if kind == "random":
        return noise(n)
    if kind == "random-then-repetitive":                # the first two segments hold no match
        return noise(min(n, 2 * S)) + rep(max(0, n - 2 * S))
    if kind == "repetitive-then-random":                # nor does the last one
        return rep(max(0, n - S)) + noise(min(n, S))
    if kind == "period3":
        return (b"xyz" * (n // 3 + 1))[:n]
    out, row = bytearray(), 0
    while len(out) < n:
        if kind == "words":
            out += WORDS[int(rng.integers(0, 16))].encode() + b" "
        else:
            out += f"{row},{WORDS[int(rng.integers(0, 16))]},{int(rng.integers(0, 1000))}.5\n".encode()
            row += 1
    return bytes(out[:n])


_BODIES = {}


def _bodies():
    """Every size with every content, made once and shared."""
    if not _BODIES:
        for n in SIZES:
            for kind in CONTENTS:
                _BODIES[(kind, n)] = _content(kind, n)
    return _BODIES


def _conditions(kind, n, size):
    from alluxio_amd.ops.native import lib
    assert 1 <= size <= lib().lz4_compress_bound(n), (kind, n, size)
    if n == 0:
        assert size == 1
    if kind == "constant" and n >= 4096:
        # 1/255 for the length bytes of the matches plus about 8 bytes per 32 KiB segment
        assert size * 100 < n, (kind, n, size)
    if kind in ("words", "csv") and n >= 4095:
        assert size < n, (kind, n, size)


def _run_direct(device, segment=S):
    """parquet_encode_lz4_raw on bodies at odd offsets of one buffer: parse and link, the sizes,
    merge; every block decodes with the host decoder to its body.  Returns the blocks by
    (content, size)."""
    import torch
    from alluxio_amd.ops.native import lib
    C = lib()
    bodies = _bodies()
    src, places = bytearray(), []
    for i, b in enumerate(bodies.values()):
        src += b"\xEE" * (1 + i % 3)                    # headers lie between bodies: every byte phase
        places.append((len(src), len(b)))
        src += b
    pages, segs, scratch_bytes = lz4_block_tables(places, segment)
    assert set((pages[:, 0] % 4).tolist()) == {0, 1, 2, 3}
    dev = torch.device(device)
    idx = dev.index if dev.type == "cuda" and dev.index is not None else 0
    num, stream = (idx, int(torch.cuda.current_stream(dev).cuda_stream)) if dev.type == "cuda" else (-1, 0)
    t_src = torch.from_numpy(np.frombuffer(bytes(src), dtype=np.uint8).copy()).to(dev)
    t_pages, t_segs = torch.from_numpy(pages).to(dev), torch.from_numpy(segs).to(dev)
    scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
    result = torch.zeros(len(pages), 4, dtype=torch.int64, device=dev)
    warm = min(4096, 65535 - segment)

    def run(mode, dst=None, out=None):
        C.parquet_encode_lz4_raw(mode, t_src.data_ptr(), t_src.numel(), t_pages.data_ptr(), len(pages), t_segs.data_ptr(),
                                 len(segs), scratch.data_ptr(), scratch_bytes, result.data_ptr(),
                                 0 if dst is None else dst.data_ptr(), 0 if out is None else out.data_ptr(),
                                 0 if out is None else out.numel(), warm, segment, num, stream)

    before = _launches()
    run(0)
    host = result.cpu().numpy()
    assert not host[:, 3].any(), host[:, 3]
    sizes = host[:, 0]
    dst = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    t_dst = torch.from_numpy(dst[:-1].copy()).to(dev)
    out = torch.full((int(dst[-1]) + 1,), 0xAA, dtype=torch.uint8, device=dev)
    run(1, t_dst, out[:-1])
    assert _launches() - before == (3 if dev.type == "cuda" else 0)
    blob = out.cpu().numpy().tobytes()
    assert blob[-1] == 0xAA                             # nothing behind the last block
    got = {}
    for (key, body), a, size in zip(bodies.items(), dst[:-1], sizes):
        block = blob[int(a):int(a) + int(size)]
        print(key, "->", int(size))
        assert C.lz4_decompress(block, len(body)) == body, key
        _conditions(key[0], key[1], int(size))
        if key[1] == 0:
            assert block == b"\x00"
        got[key] = block
    # a table row outside its buffer is refused (host: before anything runs)
    if dev.type == "cpu":
        from alluxio_amd.ops.native import native_errors
        bad = segs.copy()
        bad[-1, 3] += 1
        t_bad = torch.from_numpy(bad)
        with pytest.raises(Exception, match="segment"):
            with native_errors():
                C.parquet_encode_lz4_raw(0, t_src.data_ptr(), t_src.numel(), t_pages.data_ptr(), len(pages), t_bad.data_ptr(),
                                         len(segs), scratch.data_ptr(), scratch_bytes, result.data_ptr(), 0, 0, 0, warm, segment, -1, 0)
        with pytest.raises(Exception, match="outside the output"):
            with native_errors():
                run(1, t_dst, out[:-2])
    return got


def _text_of(kind, n, seed):
    return _content(kind, n, seed, ascii_only=True).decode("ascii")


def _sizes_spec():
    """Required columns written one row per page, so that a page body is a chosen size: a text
    value of n - 4 bytes gives n (12, 13, 4095, S - 1, S, S + 1, 2S + 1, 10S + 7), a boolean gives 1.
    The empty body is the dictionary page of ``_run_empty_dictionary``."""
    lens = [n - 4 for n in SIZES if n >= 4]
    rows = len(lens)
    spec = [(kind.replace("-", "_"), "text", [_text_of(kind, n, 1) for n in lens]) for kind in CONTENTS]
    spec.append(("flag", "bool", [bool(r % 2) for r in range(rows)]))
    return spec


def _chunk_starts(md):
    return [(cc.dictionary_page_offset if cc.dictionary_page_offset is not None else cc.data_page_offset, cc)
            for rg in md.row_groups for cc in rg.columns]


def _lz4_metadata(fs, path, md, blob, plain_blob):
    """pyarrow sees LZ4 everywhere, uncompressed sizes as in the uncompressed file, compressed sizes
    as the bytes between the chunks."""
    ref, plain = pq.ParquetFile(io.BytesIO(blob)).metadata, pq.ParquetFile(io.BytesIO(plain_blob)).metadata
    assert md == parquet_metadata(fs, path)
    starts = _chunk_starts(md)
    footer = len(blob) - 8 - int.from_bytes(blob[-8:-4], "little")
    ends = [s for s, _ in starts[1:]] + [footer]
    for (start, cc), end in zip(starts, ends):
        assert cc.codec == "LZ4_RAW" and cc.total_compressed_size == end - start, cc
    for g in range(ref.num_row_groups):
        rr, pr = ref.row_group(g), plain.row_group(g)
        assert rr.total_byte_size == pr.total_byte_size
        for j in range(rr.num_columns):
            rc, pc, cc = rr.column(j), pr.column(j), md.row_groups[g].columns[j]
            assert rc.compression == "LZ4", rc.compression
            assert rc.total_uncompressed_size == pc.total_uncompressed_size == pc.total_compressed_size
            assert rc.total_compressed_size == cc.total_compressed_size
            assert rc.data_page_offset == cc.data_page_offset


def _both_readers(fs, path, spec, device, required=()):
    blob = _read(fs, path)
    want = _arrow(spec, required)
    _same(pq.read_table(io.BytesIO(blob)), want)
    _check(read_parquet_columns(fs, path, device=device), want)
    return blob


def _run_page_sizes(c, device):
    fs = c.client()
    spec = _sizes_spec()
    names = [name for name, _k, _v in spec]
    _cols, md, blob = _write_spec(fs, "/z/sizes.parquet", spec, device, required=names, page_rows=1, compression="lz4_raw")
    _check(read_parquet_columns(fs, "/z/sizes.parquet", device=device), _arrow(spec, names))
    _cols, _md, plain = _write_spec(fs, "/z/sizes-plain.parquet", spec, device, required=names, page_rows=1)
    _lz4_metadata(fs, "/z/sizes.parquet", md, blob, plain)
    by_name = {cc.name: cc.total_compressed_size for cc in md.row_groups[0].columns}
    raw = {cc.name: cc.total_compressed_size for cc in parquet_metadata(fs, "/z/sizes-plain.parquet").row_groups[0].columns}
    print({k: (raw[k], v) for k, v in by_name.items()})
    assert by_name["constant"] * 100 < raw["constant"]
    assert by_name["words"] < raw["words"] and by_name["csv"] < raw["csv"]
    fs.close()


def _table_spec(n, seed=3):
    rng = np.random.default_rng(seed)
    vocab = ["alpha", "beta", "gamma", "delta"]
    words = rng.integers(0, 16, (n, 3))
    return [("i", "int64", [None if r % 11 == 3 else r * 7 - 5 for r in range(n)]),
            ("q", "int32", [None if r % 13 == 0 else r % 50 for r in range(n)]),
            ("d", "float64", [None if r % 4 == 2 else (float("nan") if r % 97 == 0 else r * 0.25 - 3) for r in range(n)]),
            ("f", "float32", [None if r % 5 == 1 else -0.0 if r % 9 == 0 else float(r % 100) for r in range(n)]),
            ("b", "bool", [None if r % 5 == 0 else bool(r % 3 == 0) for r in range(n)]),
            ("t", "text", [None if r % 7 == 3 else "" if r % 4 == 0 else " ".join(WORDS[k] for k in words[r])
                           for r in range(n)]),
            ("c", "category", [None if r % 6 == 5 else vocab[r % 4] for r in range(n)])], vocab


def _run_round_trip(c, device):
    """Nullable columns of every kind, 1 and 3 row groups, with and without statistics."""
    fs = c.client()
    n = 6000                                            # int64 pages of 48,000 bytes: two segments
    spec, vocab = _table_spec(n)
    for k, kw in enumerate((dict(), dict(row_group_rows=2000), dict(row_group_rows=2000, page_rows=700, statistics=True))):
        path = f"/z/rt-{k}.parquet"
        _cols, md, blob = _write_spec(fs, path, spec, device, vocab, compression="lz4_raw", **kw)
        assert len(md.row_groups) == (1 if k == 0 else 3)
        _check(read_parquet_columns(fs, path, device=device), _arrow(spec))
        _cols, _md, plain = _write_spec(fs, f"/z/rt-plain-{k}.parquet", spec, device, vocab, **kw)
        _lz4_metadata(fs, path, md, blob, plain)
        assert len(blob) < len(plain)
        if kw.get("statistics"):
            ref = pq.ParquetFile(io.BytesIO(blob)).metadata.row_group(1).column(0).statistics
            vals = [v for v in spec[0][2][2000:4000] if v is not None]
            assert (ref.min, ref.max, ref.null_count) == (min(vals), max(vals), 2000 - len(vals))
    fs.close()


def _run_big_page(c, device):
    """40,000 int64 rows in one page (about 10 segments), and 'lz4' as pyarrow spells the codec."""
    fs = c.client()
    n = 40000
    rng = np.random.default_rng(5)
    spec = [("i", "int64", [int(v) for v in rng.integers(0, 1000, n)]),
            ("r", "int64", [int(v) for v in rng.integers(-2 ** 62, 2 ** 62, n)])]
    cols = FieldColumns([_col(name, kind, vals, device) for name, kind, vals in spec])
    md = write_parquet_columns(fs, "/z/big.parquet", cols, required=["i", "r"], write_type="MUST_CACHE", compression="lz4")
    blob = _read(fs, "/z/big.parquet")
    got = pq.read_table(io.BytesIO(blob))
    back = read_parquet_columns(fs, "/z/big.parquet", device=device)
    for name, _k, vals in spec:
        assert np.array_equal(got[name].to_numpy(), np.array(vals, dtype=np.int64)), name
        assert np.array_equal(back[name].values.cpu().numpy(), np.array(vals, dtype=np.int64)), name
        assert not back[name].status.any()
    small, noise = (cc.total_compressed_size for cc in md.row_groups[0].columns)
    print("int64 pages of", 8 * n, "bytes ->", small, noise)
    # values below 1000 end in six zero bytes: at worst a token, two literals and an offset per value
    # (5 bytes of 8), plus the length bytes and the segment boundaries
    assert small < 8 * n * 3 // 4
    assert 8 * n < noise <= 8 * n + 8 * n // 255 + 16 + 64
    fs.close()


def _run_empty_dictionary(c, device):
    """An all-null category chunk has a dictionary page without bytes: the block ``00``."""
    fs = c.client()
    vocab = ["a", "bb"]
    spec = [("c", "category", [None] * 50 + ["a", "bb"] * 25), ("i", "int64", list(range(100)))]
    _cols, md, blob = _write_spec(fs, "/z/empty-dict.parquet", spec, device, vocab, row_group_rows=50, compression="lz4_raw")
    cc = md.row_groups[0].columns[0]
    assert cc.dictionary_page_offset is not None
    head = blob[cc.dictionary_page_offset:cc.data_page_offset]
    assert head.endswith(b"\x00\x00\x00") and len(head) < 32      # the header's two struct ends, then the block
    _check(read_parquet_columns(fs, "/z/empty-dict.parquet", device=device), _arrow(spec))
    cat = read_parquet_columns(fs, "/z/empty-dict.parquet", {"c": ("c", "category")}, device=device)
    assert cat["c"].values.cpu().tolist() == [-1] * 50 + [0, 1] * 25
    fs.close()


def _run_defaults_and_refusals(c, device):
    fs = c.client()
    spec, vocab = _table_spec(500)
    cols = FieldColumns([_col(name, kind, vals, device, vocab) for name, kind, vals in spec])
    blobs, deltas = [], []
    for k, kw in enumerate((dict(), dict(compression=None), dict(compression="none"), dict(compression="uncompressed"))):
        before = _launches()
        write_parquet_columns(fs, f"/z/default-{k}.parquet", cols, page_rows=200, write_type="MUST_CACHE", **kw)
        deltas.append(_launches() - before)
        blobs.append(_read(fs, f"/z/default-{k}.parquet"))
    assert blobs[0] == blobs[1] == blobs[2] == blobs[3] and len(set(deltas)) == 1
    assert pq.ParquetFile(io.BytesIO(blobs[0])).metadata.row_group(0).column(0).compression == "UNCOMPRESSED"
    for bad in ("snappy", "zstd", "gzip", 7):
        with pytest.raises(ValueError, match="lz4_raw"):
            write_parquet_columns(fs, "/z/refused.parquet", cols, write_type="MUST_CACHE", compression=bad)
        assert not fs.exists("/z/refused.parquet")
        with pytest.raises(ValueError, match="lz4_raw"):
            ParquetWriter(fs, "/z/refused.parquet", compression=bad)
        assert not fs.exists("/z/refused.parquet")
    with ParquetWriter(fs, "/z/stream.parquet", write_type="MUST_CACHE", compression="LZ4_RAW") as w:
        w.write(cols)
        w.write(cols, row_group_rows=300)
    assert w.metadata == parquet_metadata(fs, "/z/stream.parquet")
    assert [cc.codec for rg in w.metadata.row_groups for cc in rg.columns] == ["LZ4_RAW"] * (3 * len(spec))
    want = _arrow(spec)
    got = pq.read_table(io.BytesIO(_read(fs, "/z/stream.parquet")))
    _same(got.slice(0, 500), want)
    _same(got.slice(500), want)
    fs.close()


# ---- CPU: the host form --------------------------------------------------------------------------------
def _cpu(run):
    before = _launches()
    with _cluster("dram") as c:
        run(c, "cpu")
    assert _launches() == before


def test_lz4_direct_cpu():
    _run_direct("cpu")


@pytest.mark.parametrize("segment", [16 * 1024, 60 * 1024])
def test_lz4_direct_other_segments_cpu(segment):
    _run_direct("cpu", segment)


def test_lz4_page_sizes_cpu():
    _cpu(_run_page_sizes)


def test_lz4_round_trip_cpu():
    _cpu(_run_round_trip)


def test_lz4_big_page_cpu():
    _cpu(_run_big_page)


def test_lz4_empty_dictionary_cpu():
    _cpu(_run_empty_dictionary)


def test_lz4_defaults_and_refusals_cpu():
    _cpu(_run_defaults_and_refusals)


def test_lz4_bound_and_codec_names():
    """The bound that the layout refuses pages by (2^31, as lz4_block_host.h's kLbMaxLen) and the
    spellings of the codec; a page of that size is not built here."""
    from alluxio_amd.models import parquet as P
    assert P._lz4_bound(2139095040) >= 2 ** 31 > P._lz4_bound(2139095000)
    assert P._codec("LZ4") == P._codec("lz4_raw") == 7 and P._codec(None) == P._codec("NONE") == 0


def test_lz4_block_check_program(tmp_path):
    """tools/lz4_block_check.cpp builds with the command in its header and prints ok."""
    from alluxio_amd.ops.build import ROCM
    cxx = shutil.which("clang++") or os.path.join(ROCM, "lib", "llvm", "bin", "clang++")
    exe = str(tmp_path / "lz4_block_check")
    header = open(os.path.join(ROOT, "tools", "lz4_block_check.cpp")).read().split("#include")[0]
    flags = "-std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined"
    sources = "tools/lz4_block_check.cpp alluxio_amd/csrc/cpu_codecs.cpp"
    assert flags in header and "-Ialluxio_amd/csrc " + sources in header
    subprocess.run([cxx, *flags.split(), "-Ialluxio_amd/csrc", *sources.split(), "-o", exe], cwd=ROOT, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---- GPU: the kernels ----------------------------------------------------------------------------------
def _gpu(run):
    before = _launches()
    with _cluster("hbm:0") as c:
        run(c, "cuda")
    assert _launches() > before


@pytest.mark.gpu
def test_lz4_direct(gpu):
    _run_direct("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("segment", [16 * 1024, 60 * 1024])
def test_lz4_direct_other_segments(gpu, segment):
    _run_direct("cuda", segment)


@pytest.mark.gpu
def test_lz4_page_sizes(gpu):
    _gpu(_run_page_sizes)


@pytest.mark.gpu
def test_lz4_round_trip(gpu):
    _gpu(_run_round_trip)


@pytest.mark.gpu
def test_lz4_big_page(gpu):
    _gpu(_run_big_page)


@pytest.mark.gpu
def test_lz4_empty_dictionary(gpu):
    _gpu(_run_empty_dictionary)


@pytest.mark.gpu
def test_lz4_defaults_and_refusals(gpu):
    _gpu(_run_defaults_and_refusals)


@pytest.mark.gpu
def test_lz4_launch_counter(gpu):
    """Compression adds the same launches per row group for one column and for eight."""
    with _cluster("hbm:0") as c:
        fs = c.client()
        n = 3000
        kinds = ["int64", "int32", "float64", "float32", "int64", "int32", "float64", "float32"]
        eight = FieldColumns([_col(f"c{k}", kind, [None if (r + k) % 9 == 0 else r for r in range(n)], "cuda")
                              for k, kind in enumerate(kinds)])
        deltas = {}
        for name, cols in (("eight", eight), ("one", FieldColumns([eight[0]]))):
            for comp in (None, "lz4_raw"):
                before = _launches()
                write_parquet_columns(fs, f"/z/{name}-{comp}.parquet", cols, write_type="MUST_CACHE", compression=comp)
                deltas[(name, comp)] = _launches() - before
        extra = deltas[("one", "lz4_raw")] - deltas[("one", None)]
        assert extra == deltas[("eight", "lz4_raw")] - deltas[("eight", None)] == 4
        before = _launches()
        write_parquet_columns(fs, "/z/three.parquet", eight, row_group_rows=1000, write_type="MUST_CACHE", compression="lz4_raw")
        assert _launches() - before == 3 * deltas[("eight", "lz4_raw")]
        fs.close()
