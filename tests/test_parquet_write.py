"""write_parquet_columns and ParquetWriter on a mini cluster: FieldColumns are written as Parquet
files and read back with ``pyarrow`` (the independent reader) and with ``read_parquet_columns``.
All comparisons are exact, floats as bit patterns.  CPU variants run on a DRAM-tier cluster with CPU
columns (the host loops), gpu variants on the HBM tier with CUDA columns (the kernels)."""
import csv
import io
import os
import shutil
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
from test_parquet_columns import _cluster, _table

from alluxio_amd.models import (Column, FieldColumns, ParquetWriter, TextDictionary, parquet_metadata, parquet_page_table,
                                read_delimited_columns, read_parquet_columns, write_parquet_columns)
from alluxio_amd.models.fields import BOOL, CATEGORY, FLOAT32, FLOAT64, INT32, INT64, SPAN, TEXT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = {"int64": (INT64, np.int64, pa.int64()), "int32": (INT32, np.int32, pa.int32()),
         "float64": (FLOAT64, np.float64, pa.float64()), "float32": (FLOAT32, np.float32, pa.float32()),
         "bool": (BOOL, np.bool_, pa.bool_())}


def _launches():
    from alluxio_amd.ops.native import lib
    return lib().parquet_encode_launches()


def _col(name, kind, vals, device, vocab=None, dictionary=None, status=None):
    """A Column from a list with None for nulls.  category: ``vals`` are strings of ``vocab``."""
    import torch
    st = torch.tensor([1 if v is None else 0 for v in vals] if status is None else status, dtype=torch.uint8).to(device)
    if kind == "text":
        bs = [b"" if v is None else v.encode() for v in vals]
        lens = np.array([len(b) for b in bs], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        data = torch.from_numpy(np.frombuffer(b"".join(bs), dtype=np.uint8).copy()).to(device)
        return Column(name, name, TEXT, None, torch.from_numpy(lens.astype(np.int32)).to(device), st, data,
                      torch.from_numpy(offs).to(device))
    if kind == "category":
        d = dictionary if dictionary is not None else TextDictionary.from_values([v.encode() for v in vocab], device)
        where = {v: i for i, v in enumerate(x.decode() for x in d.tolist())}
        codes = torch.tensor([-1 if v is None else where[v] for v in vals], dtype=torch.int32).to(device)
        return Column(name, name, CATEGORY, codes, None, st, dictionary=d)
    code, dt, _ = TYPES[kind]
    arr = np.array([0 if v is None else v for v in vals], dtype=dt)
    return Column(name, name, code, torch.from_numpy(arr).to(device), None, st)


def _arrow(spec, required=()):
    """The pyarrow table that a list of (name, kind, values) should read back as."""
    cols, fields = {}, []
    for name, kind, vals in spec:
        t = pa.string() if kind in ("text", "category") else TYPES[kind][2]
        cols[name] = pa.array(vals, t)
        fields.append(pa.field(name, t, nullable=name not in required))
    return pa.table(cols, schema=pa.schema(fields))


def _same(got: pa.Table, want: pa.Table):
    """Values, nulls, types and field nullability, floats as bit patterns."""
    assert got.schema.names == want.schema.names
    assert got.num_rows == want.num_rows
    for f in want.schema:
        g = got.schema.field(f.name)
        assert (g.type, g.nullable) == (f.type, f.nullable), f.name
        a, b = got[f.name].to_pylist(), want[f.name].to_pylist()
        assert [x is None for x in a] == [x is None for x in b], f.name
        if pa.types.is_floating(f.type):
            dt, it = (np.float64, np.int64) if f.type == pa.float64() else (np.float32, np.int32)
            fa, fb = (np.array([0 if x is None else x for x in v], dtype=dt).view(it) for v in (a, b))
            assert np.array_equal(fa, fb), f.name
        else:
            assert a == b, f.name


def _check(got: FieldColumns, want: pa.Table):
    """Columns read by read_parquet_columns against a pyarrow table; a null has status 1 and value 0."""
    import torch
    assert got.names == want.column_names and got.rows == want.num_rows
    for f in want.schema:
        w, c = want[f.name].to_pylist(), got[f.name]
        assert c.status.cpu().tolist() == [1 if v is None else 0 for v in w], f.name
        if pa.types.is_string(f.type):
            assert c.tolist() == [None if v is None else v.encode() for v in w], f.name
            continue
        dt, it, tt = {pa.float64(): (np.float64, np.int64, torch.float64), pa.float32(): (np.float32, np.int32, torch.float32),
                      pa.int64(): (np.int64, np.int64, torch.int64), pa.int32(): (np.int32, np.int32, torch.int32),
                      pa.bool_(): (np.bool_, np.uint8, torch.bool)}[f.type]
        assert c.values.dtype == tt, f.name
        expect = np.array([0 if v is None else v for v in w], dtype=dt)
        assert np.array_equal(c.values.cpu().numpy().view(it), expect.view(it)), f.name


def _read(fs, path):
    return fs.read_file(path)


def _pages(blob, md):
    """The page table of every chunk of a written file (host walk): {(row group, column): rows}."""
    import torch
    data = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy())
    out = {}
    for g, rg in enumerate(md.row_groups):
        for j, cc in enumerate(rg.columns):
            start = cc.dictionary_page_offset if cc.dictionary_page_offset is not None else cc.data_page_offset
            table, counts, errors = parquet_page_table(data, [start], [cc.total_compressed_size])
            assert not errors.any() and counts[0] == len(table)
            out[(g, j)] = table
    return out


def _value_offsets(blob, md, pages, j):
    """File offsets of the value areas of the data pages of column j (V1: after the level block)."""
    opt = md.schema[j].max_definition_level == 1
    offs = []
    for (g, jj), table in pages.items():
        for r in table:
            if jj == j and r[0] == 0:
                payload = int(r[1])
                offs.append(payload + (4 + int.from_bytes(blob[payload:payload + 4], "little") if opt else 0))
    return offs


def _metadata_agrees(md, blob):
    ref = pq.ParquetFile(io.BytesIO(blob)).metadata
    assert md.num_rows == ref.num_rows and len(md.row_groups) == ref.num_row_groups and md.created_by == ref.created_by
    assert "alluxio" in md.created_by
    for g, rg in enumerate(md.row_groups):
        rr = ref.row_group(g)
        assert rg.num_rows == rr.num_rows and len(rg.columns) == rr.num_columns
        for j, cc in enumerate(rg.columns):
            rc = rr.column(j)
            assert (cc.name, cc.physical_type, cc.codec, cc.num_values, cc.data_page_offset, cc.total_compressed_size,
                    cc.dictionary_page_offset) == \
                   (rc.path_in_schema, rc.physical_type, rc.compression, rc.num_values, rc.data_page_offset,
                    rc.total_compressed_size, rc.dictionary_page_offset if rc.has_dictionary_page else None)
            assert rc.statistics is None and rc.total_uncompressed_size == rc.total_compressed_size


def _to(cols: FieldColumns, device) -> FieldColumns:
    """The same columns with every tensor (and dictionary) on ``device``."""
    out, dicts = [], {}
    for c in cols:
        if c.type == TEXT:
            out.append(Column(c.name, c.field, TEXT, None, c.length.to(device), c.status.to(device), c.data.to(device),
                              c.offsets.to(device)))
        elif c.type == CATEGORY:
            d = dicts.setdefault(id(c.dictionary), TextDictionary.from_values(c.dictionary.tolist(), device))
            out.append(Column(c.name, c.field, CATEGORY, c.values.to(device), None, c.status.to(device), dictionary=d))
        else:
            out.append(Column(c.name, c.field, c.type, c.values.to(device), None, c.status.to(device)))
    return FieldColumns(out)


# ---- scenarios ----------------------------------------------------------------------------------------
def _run_round_trip(c, device, variants=(None,)):
    from alluxio_amd.ops.native import lib
    fs = c.client()
    want = _table()
    buf = io.BytesIO()
    pq.write_table(want, buf, compression="none", data_page_version="1.0")
    fs.write_file("/w/src.parquet", buf.getvalue(), write_type="MUST_CACHE")
    spec = {k: (k, "category" if k == "label" else None) for k in want.column_names}
    cols = read_parquet_columns(fs, "/w/src.parquet", spec, device=device)
    md = write_parquet_columns(fs, "/w/out.parquet", cols, row_group_rows=2000, page_rows=300, required=["seq"],
                               write_type="MUST_CACHE")
    blob = _read(fs, "/w/out.parquet")
    _same(pq.read_table(io.BytesIO(blob)), want)
    assert [rg.num_rows for rg in md.row_groups] == [2000, 2000, 1000]
    assert md == parquet_metadata(fs, "/w/out.parquet")
    _metadata_agrees(md, blob)
    pages = _pages(blob, md)
    assert all(len([r for r in t if r[0] == 0]) == -(-md.row_groups[g].num_rows // 300) for (g, _j), t in pages.items())
    default = lib().parquet_decode_variant()
    try:
        for v in variants:
            if v is not None:
                lib().set_parquet_decode_variant(v)
            back = read_parquet_columns(fs, "/w/out.parquet", device=device)
            _check(back, want)
            cat = read_parquet_columns(fs, "/w/out.parquet", {"label": ("label", "category")}, device=device)
            assert cat["label"].values.cpu().tolist() == cols["label"].values.cpu().tolist()
    finally:
        lib().set_parquet_decode_variant(default)
    fs.close()
    return blob


def _edge_spec(n, seed=0):
    rng = np.random.default_rng(seed + n)
    i64 = [-2 ** 63, 2 ** 63 - 1, 0, -1, 1]
    i32 = [-2 ** 31, 2 ** 31 - 1, 0, -1]
    vocab = ["a", "bb", "ccc"]
    return [("i", "int64", [None if r % 3 == 1 else i64[r % 5] for r in range(n)]),
            ("q", "int32", [i32[r % 4] for r in range(n)]),
            ("b", "bool", [None if r % 5 == 0 else bool(rng.integers(0, 2)) for r in range(n)]),
            ("t", "text", [None if r % 7 == 3 else "" if r % 4 == 0 else "é" * (r % 9) + str(r) for r in range(n)]),
            ("c", "category", [None if r % 6 == 5 else vocab[r % 3] for r in range(n)]),
            ("d", "float64", [None if r % 4 == 2 else float(r) * 0.5 - 3 for r in range(n)])], vocab


def _write_spec(fs, path, spec, device, vocab=None, required=(), **kw):
    cols = FieldColumns([_col(name, kind, vals, device, vocab) for name, kind, vals in spec])
    md = write_parquet_columns(fs, path, cols, required=required, write_type="MUST_CACHE", **kw)
    blob = _read(fs, path)
    _same(pq.read_table(io.BytesIO(blob)), _arrow(spec, required))
    assert md == parquet_metadata(fs, path)
    return cols, md, blob


def _run_edge_rows(c, device):
    fs = c.client()
    odd = 0
    for n in (0, 1, 7, 8, 9, 63, 64, 65, 1000):
        for pr in ((None,) if n <= 65 else (64, 100)):
            spec, vocab = _edge_spec(n)
            path = f"/w/rows-{n}-{pr}.parquet"
            cols, md, blob = _write_spec(fs, path, spec, device, vocab, required=["q"], page_rows=pr)
            assert len(md.row_groups) == (1 if n else 0)
            if pr == 64:                                # valid booleans that are no multiple of 8 in a page
                assert sum(v is not None for v in spec[2][2][:64]) % 8
            _metadata_agrees(md, blob)
            back = read_parquet_columns(fs, path, device=device)
            _check(back, _arrow(spec, ["q"]))
            if n:
                pages = _pages(blob, md)
                for j in (0, 1, 5):                     # the PLAIN fixed-width columns
                    odd += sum(o % 2 for o in _value_offsets(blob, md, pages, j))
    assert odd > 0                                      # a PLAIN value area at an odd file offset
    fs.close()


def _run_edge_nulls(c, device):
    """Pages of 64 rows: all null, no null, a null only in the first row, only in the last row, and a
    text page whose values are all empty."""
    fs = c.client()
    n = 64 * 5 + 10

    def null(r):
        p, i = divmod(r, 64)
        return p == 0 or (p == 2 and i == 0) or (p == 3 and i == 63) or (p >= 4 and r % 3 == 0)

    vocab = ["x", "yy"]
    spec = [("v", "int32", [None if null(r) else r - 100 for r in range(n)]),
            ("f", "float32", [None if null(r) else float(np.float32(r * 0.1)) for r in range(n)]),
            ("b", "bool", [None if null(r) else r % 3 != 0 for r in range(n)]),
            ("t", "text", [None if null(r) else "" if r // 64 == 1 else f"s{r}" for r in range(n)]),
            ("c", "category", [None if null(r) else vocab[r % 2] for r in range(n)])]
    cols, md, blob = _write_spec(fs, "/w/nulls.parquet", spec, device, vocab, page_rows=64)
    _check(read_parquet_columns(fs, "/w/nulls.parquet", device=device), _arrow(spec))
    # the level streams: page 1 has no null and is one RLE run (header 64 << 1, value 1)
    pages = _pages(blob, md)
    for j in range(len(spec)):
        data = [r for r in pages[(0, j)] if r[0] == 0]
        assert len(data) == 6
        p1 = int(data[1][1])
        assert blob[p1:p1 + 7] == b"\x03\x00\x00\x00\x80\x01\x01"
        p0 = int(data[0][1])
        assert blob[p0:p0 + 5] == b"\x09\x00\x00\x00\x11" and blob[p0 + 5:p0 + 13] == bytes(8)   # all null: 8 zero bytes
        p5 = int(data[5][1])                            # 10 rows: 2 bytes, zero padding bits
        assert blob[p5:p5 + 5] == b"\x03\x00\x00\x00\x05" and blob[p5 + 6] >> 2 == 0
    fs.close()


def _run_edge_dictionaries(c, device):
    fs = c.client()
    n = 700
    for entries, width in ((1, 1), (2, 1), (3, 2), (256, 8), (257, 9)):
        vocab = [f"v{k}" for k in range(entries)]
        spec = [("c", "category", [None if r % 10 == 9 else vocab[(r * 7) % entries] for r in range(n)])]
        path = f"/w/dict-{entries}.parquet"
        cols, md, blob = _write_spec(fs, path, spec, device, vocab, page_rows=300)
        pages = _pages(blob, md)[(0, 0)]
        dict_pages = [r for r in pages if r[0] == 2]
        assert len(dict_pages) == 1 and dict_pages[0][4] == entries and dict_pages[0][5] == 0      # PLAIN
        for off, r in zip(_value_offsets(blob, md, {(0, 0): pages}, 0), [r for r in pages if r[0] == 0]):
            assert blob[off] == width and r[5] == 8     # RLE_DICTIONARY
        got = read_parquet_columns(fs, path, {"c": ("c", "category")}, device=device)
        words = got["c"].dictionary.tolist()           # the reader's codes are in order of first occurrence
        assert [None if k < 0 else words[k].decode() for k in got["c"].values.cpu().tolist()] == spec[0][2]
        _check(read_parquet_columns(fs, path, device=device), _arrow(spec))
    # one dictionary, two row groups, the second uses higher codes
    vocab = [f"w{k}" for k in range(7)]
    spec = [("c", "category", [vocab[r % 2] if r < 100 else vocab[2 + r % 5] for r in range(200)]),
            ("b", "bool", [r % 3 == 0 for r in range(200)])]
    cols, md, blob = _write_spec(fs, "/w/dict-shared.parquet", spec, device, vocab, row_group_rows=100)
    pages = _pages(blob, md)
    assert [[r[4] for r in pages[(g, 0)] if r[0] == 2] for g in (0, 1)] == [[2], [7]]
    fs.close()


def _run_csv(c, device):
    fs = c.client()
    kinds = ["red", "green", "blue, dark"]
    rows = [[i, f"{i * 1.25 - 7:.2f}" if i % 9 else "1e-320", f'name "{i}", é' if i % 4 else "", kinds[i % 3]]
            for i in range(300)]
    buf = io.StringIO()
    w = csv.writer(buf, lineterminator="\n")
    w.writerow(["id", "price", "name", "kind"])
    w.writerows(rows)
    text = buf.getvalue()
    fs.write_file("/w/in.csv", text.encode(), write_type="MUST_CACHE")
    cols = read_delimited_columns(fs, "/w/in.csv", {"id": ("id", "int64"), "price": ("price", "float64"),
                                                    "name": ("name", "text"), "kind": ("kind", "category")},
                                  quote='"', header=True, device=device)
    write_parquet_columns(fs, "/w/from-csv.parquet", cols, write_type="MUST_CACHE")
    got = pq.read_table(io.BytesIO(_read(fs, "/w/from-csv.parquet")))
    read = list(csv.reader(io.StringIO(text)))[1:]
    want = [("id", "int64", [int(r[0]) for r in read]), ("price", "float64", [float(r[1]) for r in read]),
            ("name", "text", [r[2] or None for r in read]), ("kind", "category", [r[3] for r in read])]
    _same(got, _arrow(want))
    fs.close()


def _run_streaming(c, device):
    fs = c.client()
    vocab = ["a", "b", "c", "d"]
    d = TextDictionary.from_values([v.encode() for v in vocab], device)
    parts = [[("n", "int64", [k * 100 + r for r in range(50 + k)]),
              ("c", "category", [None if r % 5 == 1 else vocab[(r + k) % (2 + k)] for r in range(50 + k)])] for k in range(3)]
    with ParquetWriter(fs, "/w/stream.parquet", write_type="MUST_CACHE") as w:
        for spec in parts:
            w.write(FieldColumns([_col(name, kind, vals, device, dictionary=d) for name, kind, vals in spec]))
        assert w.metadata is None
        with pytest.raises(ValueError, match="differ"):
            w.write(FieldColumns([_col("n", "int32", [1], device), _col("c", "category", ["a"], device, dictionary=d)]))
        with pytest.raises(ValueError, match="differ"):
            w.write(FieldColumns([_col("m", "int64", [1], device), _col("c", "category", ["a"], device, dictionary=d)]))
    md = w.metadata
    blob = _read(fs, "/w/stream.parquet")
    assert [rg.num_rows for rg in md.row_groups] == [50, 51, 52] and md == parquet_metadata(fs, "/w/stream.parquet")
    assert blob.count(b"PAR1") == 2 and pq.ParquetFile(io.BytesIO(blob)).metadata.num_row_groups == 3
    whole = [(name, kind, sum((p[j][2] for p in parts), [])) for j, (name, kind, _v) in enumerate(parts[0])]
    _same(pq.read_table(io.BytesIO(blob)), _arrow(whole))
    fs.close()


def _run_refusals(c, device):
    import torch
    fs = c.client()
    n = 20
    ok = _col("a", "int64", list(range(n)), device)

    def refused(exc, match, cols, **kw):
        path = f"/w/refused-{refused.k}.parquet"
        refused.k += 1
        with pytest.raises(exc, match=match):
            write_parquet_columns(fs, path, FieldColumns(cols), write_type="MUST_CACHE", **kw)
        assert not fs.exists(path)
        return path

    refused.k = 0
    span = Column("s", 0, SPAN, torch.zeros(n, dtype=torch.int64, device=device),
                  torch.zeros(n, dtype=torch.int32, device=device), torch.zeros(n, dtype=torch.uint8, device=device))
    refused(TypeError, "'s'.*span", [ok, span])
    st = [0] * n
    st[7] = 2
    malformed = _col("m", "int32", list(range(n)), device, status=st)
    refused(ValueError, "'m'.*status", [ok, malformed])
    st[7] = 3
    deferred = _col("fl", "float64", [float(r) for r in range(n)], device, status=st)
    refused(ValueError, "'fl'.*status", [ok, deferred])
    # invalid="null": such rows become nulls
    write_parquet_columns(fs, "/w/as-null.parquet", FieldColumns([ok, deferred]), invalid="null", write_type="MUST_CACHE")
    got = pq.read_table(io.BytesIO(_read(fs, "/w/as-null.parquet")))
    assert got["fl"].to_pylist() == [None if r == 7 else float(r) for r in range(n)]
    refused(ValueError, "'fl'.*required", [ok, deferred], invalid="null", required=["fl"])
    nullable = _col("x", "int64", [None if r == n - 1 else r for r in range(n)], device)
    refused(ValueError, "'x'.*required.*1 null", [ok, nullable], required=["x"])
    cat = _col("c", "category", ["u", "v"] * (n // 2), device, vocab=["u", "v"])
    cat.values[3] = 2
    refused(ValueError, "'c'.*outside its dictionary", [ok, cat])
    cat.values[3] = -1
    refused(ValueError, "'c'.*outside its dictionary", [ok, cat])
    # a page body of 2^31 bytes or more: two text values of 2^30 bytes (the data is never touched)
    big = Column("big", "big", TEXT, None, torch.full((2,), 2 ** 30, dtype=torch.int32, device=device),
                 torch.zeros(2, dtype=torch.uint8, device=device), torch.empty(2 ** 31, dtype=torch.uint8, device=device),
                 torch.tensor([0, 2 ** 30, 2 ** 31], dtype=torch.int64, device=device))
    refused(ValueError, "'big'.*2\\^31", [big])
    del big
    # the streaming writer: a refused first call creates nothing, a refused later call leaves the file usable
    w = ParquetWriter(fs, "/w/refused-stream.parquet", write_type="MUST_CACHE")
    with pytest.raises(ValueError, match="'m'"):
        w.write(FieldColumns([malformed]))
    w.close()
    assert not fs.exists("/w/refused-stream.parquet")
    fs.close()


# ---- CPU ----------------------------------------------------------------------------------------------
def _cpu(run):
    before = _launches()
    with _cluster("dram") as c:
        out = run(c, "cpu")
    assert _launches() == before                        # the host loops
    return out


def test_write_round_trip_cpu():
    _cpu(_run_round_trip)


def test_write_edge_rows_cpu():
    _cpu(_run_edge_rows)


def test_write_edge_nulls_cpu():
    _cpu(_run_edge_nulls)


def test_write_edge_dictionaries_cpu():
    _cpu(_run_edge_dictionaries)


def test_write_csv_cpu():
    _cpu(_run_csv)


def test_write_streaming_cpu():
    _cpu(_run_streaming)


def test_write_refusals_cpu():
    _cpu(_run_refusals)


def test_encode_check_program(tmp_path):
    """tools/parquet_encode_check.cpp builds with the command in its header and prints ok."""
    from alluxio_amd.ops.build import ROCM
    cxx = shutil.which("clang++") or os.path.join(ROCM, "lib", "llvm", "bin", "clang++")
    exe = str(tmp_path / "parquet_encode_check")
    header = open(os.path.join(ROOT, "tools", "parquet_encode_check.cpp")).read().split("#include")[0]
    flags = "-std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined"
    assert flags in header and "-Ialluxio_amd/csrc tools/parquet_encode_check.cpp" in header
    subprocess.run([cxx, *flags.split(), "-Ialluxio_amd/csrc", "tools/parquet_encode_check.cpp", "-o", exe], cwd=ROOT,
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---- GPU ----------------------------------------------------------------------------------------------
def _gpu(run, **kw):
    before = _launches()
    with _cluster("hbm:0") as c:
        out = run(c, "cuda", **kw)
    assert _launches() > before                         # the kernels
    return out


@pytest.mark.gpu
def test_write_round_trip(gpu):
    _gpu(_run_round_trip, variants=(0, 1))


@pytest.mark.gpu
def test_write_edge_rows(gpu):
    _gpu(_run_edge_rows)


@pytest.mark.gpu
def test_write_edge_nulls(gpu):
    _gpu(_run_edge_nulls)


@pytest.mark.gpu
def test_write_edge_dictionaries(gpu):
    _gpu(_run_edge_dictionaries)


@pytest.mark.gpu
def test_write_csv(gpu):
    _gpu(_run_csv)


@pytest.mark.gpu
def test_write_streaming(gpu):
    _gpu(_run_streaming)


@pytest.mark.gpu
def test_write_refusals(gpu):
    _gpu(_run_refusals)


@pytest.mark.gpu
def test_write_same_bytes(gpu):
    """The file written from CUDA columns equals, byte for byte, the one from the same columns on the CPU."""
    with _cluster("hbm:0") as c:
        fs = c.client()
        want = _table()
        buf = io.BytesIO()
        pq.write_table(want, buf, compression="none")
        fs.write_file("/w/src.parquet", buf.getvalue(), write_type="MUST_CACHE")
        spec = {k: (k, "category" if k == "label" else None) for k in want.column_names}
        cols = read_parquet_columns(fs, "/w/src.parquet", spec, device="cuda")
        for k, kw in enumerate((dict(row_group_rows=2000, page_rows=300, required=["seq"]), dict(page_rows=1000), {})):
            before = _launches()
            write_parquet_columns(fs, f"/w/dev-{k}.parquet", cols, write_type="MUST_CACHE", **kw)
            mid = _launches()
            write_parquet_columns(fs, f"/w/host-{k}.parquet", _to(cols, "cpu"), write_type="MUST_CACHE", **kw)
            assert mid > before and _launches() == mid
            assert _read(fs, f"/w/dev-{k}.parquet") == _read(fs, f"/w/host-{k}.parquet")
        spec, vocab = _edge_spec(1000)
        for pr in (64, 100):
            dev = FieldColumns([_col(name, kind, vals, "cuda", vocab) for name, kind, vals in spec])
            write_parquet_columns(fs, f"/w/edge-dev-{pr}.parquet", dev, page_rows=pr, write_type="MUST_CACHE")
            write_parquet_columns(fs, f"/w/edge-host-{pr}.parquet", _to(dev, "cpu"), page_rows=pr, write_type="MUST_CACHE")
            assert _read(fs, f"/w/edge-dev-{pr}.parquet") == _read(fs, f"/w/edge-host-{pr}.parquet")
        fs.close()


@pytest.mark.gpu
def test_write_launch_counter(gpu):
    """No launch for a write without rows; the launches of a row group do not grow with its columns."""
    with _cluster("hbm:0") as c:
        fs = c.client()
        n = 3000
        before = _launches()
        write_parquet_columns(fs, "/w/none.parquet", FieldColumns([_col("a", "int64", [], "cuda")]), write_type="MUST_CACHE")
        assert _launches() == before
        kinds = ["int64", "int32", "float64", "float32", "int64", "int32", "float64", "float32"]
        eight = FieldColumns([_col(f"c{k}", kind, [None if (r + k) % 9 == 0 else r for r in range(n)], "cuda")
                              for k, kind in enumerate(kinds)])
        write_parquet_columns(fs, "/w/eight.parquet", eight, write_type="MUST_CACHE")
        mid = _launches()
        write_parquet_columns(fs, "/w/one.parquet", FieldColumns([eight[0]]), write_type="MUST_CACHE")
        assert mid - before == _launches() - mid > 0
        fs.close()
