"""read_parquet_columns, parquet_row_groups and parquet_metadata on a mini cluster: one pyarrow
table of 5,000 rows (ints, a nullable int32, floats with NaN, infinities and -0.0, a nullable bool,
a nullable label with 13 distinct values, a distinct text of 0 to 40 bytes with multi-byte UTF-8
and empty strings, a non-nullable int64) written in six forms and read back; every column must
equal what ``pq.read_table`` gives.  CPU variants run on a DRAM-tier cluster (the host loops), gpu
variants on the HBM tier (the kernels, in both variants of the hybrid decode)."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from alluxio_amd.minicluster import LocalAlluxioCluster
from alluxio_amd.models import (FieldColumns, TextDictionary, parquet_metadata, parquet_page_table, parquet_row_groups,
                                read_parquet_columns)

NROWS = 5000
PIECES = ["a", "b", "é", "\U0001f600", "ß", " ", "x y", "\n", "日本", "z"]
FORMS = {"v1": dict(data_page_version="1.0", compression="none"),
         "v2": dict(data_page_version="2.0", compression="none"),
         "v1-lz4": dict(data_page_version="1.0", compression="lz4"),
         "v2-lz4": dict(data_page_version="2.0", compression="lz4"),
         "plain": dict(use_dictionary=False, compression="none"),
         "dict-limit": dict(dictionary_pagesize_limit=2048, compression="none")}


def _cluster(path):
    return LocalAlluxioCluster(num_workers=1, conf={"alluxio.worker.tieredstore.level0.dirs.path": path,
                                                    "alluxio.worker.hbm.page.size": "64KB",
                                                    "alluxio.user.block.size.bytes.default": "256KB"})


def _text(rng, r):
    if r % 50 == 7:
        return ""
    s = f"{r}:" + "".join(PIECES[i] for i in rng.integers(0, len(PIECES), int(rng.integers(0, 12))))
    while len(s.encode()) > 40:
        s = s[:-1]
    return s


def _table(n=NROWS, seed=4):
    rng = np.random.default_rng(seed)
    score = rng.standard_normal(n) * 1e3
    if n:
        score[[3 % n, 500 % n, 2001 % n, 4999 % n]] = [np.nan, np.inf, -np.inf, -0.0]
    cols = {"id": pa.array(np.arange(n, dtype=np.int64) * 7919 - 10 ** 12, pa.int64()),
            "count": pa.array([None if r % 11 == 3 else int(rng.integers(-2 ** 31, 2 ** 31)) for r in range(n)], pa.int32()),
            "score": pa.array(score, pa.float64()),
            "f32": pa.array(rng.standard_normal(n).astype(np.float32), pa.float32()),
            "ok": pa.array([None if r % 13 == 5 else bool(rng.integers(0, 2)) for r in range(n)], pa.bool_()),
            "label": pa.array([None if r % 17 == 2 else f"t{(r * 5 + seed) % 13}" for r in range(n)], pa.string()),
            "text": pa.array([_text(rng, r) for r in range(n)], pa.string()),
            "seq": pa.array(np.arange(n, dtype=np.int64) % 97, pa.int64())}
    schema = pa.schema([pa.field(k, v.type, nullable=k != "seq") for k, v in cols.items()])
    return pa.table(cols, schema=schema)


_BLOBS = {}


def _blob(form):
    if form not in _BLOBS:
        buf = io.BytesIO()
        pq.write_table(_table(), buf, row_group_size=2000, data_page_size=4096, **FORMS[form])
        _BLOBS[form] = buf.getvalue()
    return _BLOBS[form]


def _np(t):
    return t.cpu().numpy()


def _codes(values):
    d = {}
    return [-1 if v is None else d.setdefault(v, len(d)) for v in values], d


def _check(got: FieldColumns, want: pa.Table, names=None):
    import torch
    names = names or want.column_names
    assert got.rows == want.num_rows
    for k in names:
        w, c = want[k].to_pylist(), got[k]
        st = _np(c.status)
        assert st.tolist() == [1 if v is None else 0 for v in w], k
        t = want.schema.field(k).type
        if pa.types.is_floating(t):
            iv, fv = (np.int64, np.float64) if t == pa.float64() else (np.int32, np.float32)
            assert c.values.dtype == (torch.float64 if t == pa.float64() else torch.float32)
            assert np.array_equal(_np(c.values).view(iv), np.array(w, dtype=fv).view(iv)), k
        elif pa.types.is_string(t):
            assert c.tolist() == [None if v is None else v.encode() for v in w], k
            assert _np(c.length).tolist() == [0 if v is None else len(v.encode()) for v in w], k
        else:
            assert c.values.dtype == {pa.int64(): torch.int64, pa.int32(): torch.int32, pa.bool_(): torch.bool}[t]
            assert c.tolist() == w, k
            assert not _np(c.values)[st != 0].any(), k  # a null has value 0


def _run_forms(c, device, form):
    import torch
    fs = c.client()
    blob = _blob(form)
    path = f"/pq/{form}.parquet"
    fs.write_file(path, blob, write_type="MUST_CACHE")
    want = pq.read_table(io.BytesIO(blob))
    got = read_parquet_columns(fs, path, device=device)
    assert got.names == want.column_names and got["id"].values.device.type == torch.device(device).type
    _check(got, want)
    md = parquet_metadata(fs, path)
    assert len(md.row_groups) == 3
    if form == "dict-limit":
        # the form proves something only if a chunk really holds dictionary-coded and PLAIN data pages
        mixed = 0
        for rg in md.row_groups:
            for cc in rg.columns:
                start = cc.dictionary_page_offset or cc.data_page_offset
                chunk = torch.from_numpy(np.frombuffer(blob[start:start + cc.total_compressed_size], dtype=np.uint8).copy())
                table, counts, errors = parquet_page_table(chunk.to(device), [0], [chunk.numel()])
                assert not errors.any() and counts[0] == len(table)
                encs = set(table[table[:, 0] != 2][:, 5].tolist())
                mixed += bool(encs & {2, 8}) and 0 in encs
        assert mixed >= 3
    # categories: codes through the vocabulary, in first-occurrence order
    cat = read_parquet_columns(fs, path, {"label": ("label", "category"), "t": ("text", "category"), "n": ("seq", "int64")},
                               device=device)
    for name, leaf in (("label", "label"), ("t", "text")):
        codes, d = _codes(want[leaf].to_pylist())
        assert _np(cat[name].values).tolist() == codes, (form, name)
        assert cat[name].dictionary.tolist() == [v.encode() for v in d]
        assert cat[name].values.dtype == torch.int32
    assert len(cat["label"].dictionary) == 13
    fs.close()


def _run_interface(c, device):
    import torch
    fs = c.client()
    blob = _blob("v1")
    fs.write_file("/pq/a.parquet", blob, write_type="MUST_CACHE")
    want = pq.read_table(io.BytesIO(blob))
    # row groups in the order asked for; a list of columns; a dict; widening
    got = read_parquet_columns(fs, "/pq/a.parquet", ["text", "count", "ok"], row_groups=[2, 0], device=device)
    assert got.names == ["text", "count", "ok"]
    _check(got, pa.concat_tables([want.slice(4000, 1000), want.slice(0, 2000)]), ["text", "count", "ok"])
    wide = read_parquet_columns(fs, "/pq/a.parquet", {"c64": ("count", "int64"), "f64": ("f32", "float64"),
                                                      "c": ("count", "int32"), "b": ("ok", "bool")}, device=device)
    assert wide["c64"].values.dtype == torch.int64 and wide["f64"].values.dtype == torch.float64
    assert wide["c64"].tolist() == want["count"].to_pylist() == wide["c"].tolist() and wide["b"].tolist() == want["ok"].to_pylist()
    assert np.array_equal(_np(wide["f64"].values).view(np.int64),
                          np.array(want["f32"].to_pylist(), dtype=np.float32).astype(np.float64).view(np.int64))
    same = read_parquet_columns(fs, "/pq/a.parquet", device=device, device_plan=False)
    _check(same, want)
    # parquet_row_groups: one part per row group, one dictionary for all
    parts = list(parquet_row_groups(fs, "/pq/a.parquet", {"label": ("label", "category"), "id": ("id", None)}, device=device))
    assert [p.rows for p in parts] == [2000, 2000, 1000] and len({id(p["label"].dictionary) for p in parts}) == 1
    whole = FieldColumns.concat(parts)
    assert _np(whole["label"].values).tolist() == _codes(want["label"].to_pylist())[0]
    assert whole["id"].tolist() == want["id"].to_pylist()
    # one dictionary shared by two files
    other = _table(n=300, seed=9)
    buf = io.BytesIO()
    pq.write_table(other, buf, compression="lz4", data_page_version="2.0")
    fs.write_file("/pq/b.parquet", buf.getvalue(), write_type="MUST_CACHE")
    d = TextDictionary(device)
    one = read_parquet_columns(fs, "/pq/a.parquet", {"label": ("label", "category")}, device=device, dictionaries={"label": d})
    two = read_parquet_columns(fs, "/pq/b.parquet", {"label": ("label", "category")}, device=device, dictionaries={"label": d})
    assert one["label"].dictionary is d and two["label"].dictionary is d and len(d) == 13
    vocab = d.tolist()
    assert [None if c < 0 else vocab[c].decode() for c in _np(two["label"].values)] == other["label"].to_pylist()
    assert FieldColumns.concat([one, two]).rows == NROWS + 300
    # a file with 0 rows, with and without a row group
    for k, rgs in enumerate((None, [])):
        buf = io.BytesIO()
        pq.write_table(_table(n=0), buf, compression="none")
        fs.write_file(f"/pq/empty{k}.parquet", buf.getvalue(), write_type="MUST_CACHE")
        got = read_parquet_columns(fs, f"/pq/empty{k}.parquet", row_groups=rgs, device=device)
        assert got.rows == 0 and got["score"].values.dtype == torch.float64 and got["ok"].values.dtype == torch.bool
        assert got["text"].data.numel() == 0 and got["text"].offsets.tolist() == [0]
    # error paths, before any launch
    with pytest.raises(ValueError, match="cannot be read as"):
        read_parquet_columns(fs, "/pq/a.parquet", {"x": ("id", "int32")}, device=device)
    with pytest.raises(ValueError, match="cannot be read as"):
        read_parquet_columns(fs, "/pq/a.parquet", {"x": ("score", "float32")}, device=device)
    with pytest.raises(ValueError, match="unknown column type"):
        read_parquet_columns(fs, "/pq/a.parquet", {"x": ("id", "complex")}, device=device)
    with pytest.raises(KeyError):
        read_parquet_columns(fs, "/pq/a.parquet", ["nope"], device=device)
    with pytest.raises(IndexError):
        read_parquet_columns(fs, "/pq/a.parquet", row_groups=[3], device=device)
    fs.write_file("/pq/not.parquet", b"PAR1 this is no parquet file", write_type="MUST_CACHE")
    with pytest.raises(ValueError, match="PAR1"):
        parquet_metadata(fs, "/pq/not.parquet")
    fs.close()


def _run_refusals(c, device):
    fs = c.client()
    n = 200
    base = {"id": pa.array(np.arange(n), pa.int64()), "name": pa.array([f"n{i % 5}" for i in range(n)], pa.string())}

    def put(name, tbl, **kw):
        buf = io.BytesIO()
        pq.write_table(tbl, buf, **kw)
        fs.write_file(f"/pq/{name}.parquet", buf.getvalue(), write_type="MUST_CACHE")
        return f"/pq/{name}.parquet"

    def ok(path, tbl):
        got = read_parquet_columns(fs, path, ["id", "name"], device=device)
        assert got["id"].tolist() == tbl["id"].to_pylist() and got["name"].tolist() == [v.encode() for v in tbl["name"].to_pylist()]

    from alluxio_amd.ops.native import lib
    before = lib().parquet_decode_launches()
    p = put("snappy", pa.table(base), compression="snappy")
    with pytest.raises(NotImplementedError, match="SNAPPY.*|.*'id'.*"):
        read_parquet_columns(fs, p, ["id"], device=device)
    with pytest.raises(NotImplementedError, match="SNAPPY"):
        read_parquet_columns(fs, p, device=device)
    for codec in ("gzip", "zstd"):
        with pytest.raises(NotImplementedError, match=codec.upper()):
            read_parquet_columns(fs, put(codec, pa.table(base), compression=codec), ["id"], device=device)
    nested = pa.table(dict(base, lst=pa.array([[i, i + 1] for i in range(n)], pa.list_(pa.int32()))))
    p = put("nested", nested, compression="none")
    with pytest.raises(NotImplementedError, match="lst.*repeated"):
        read_parquet_columns(fs, p, ["lst.list.element"], device=device)
    flba = pa.table(dict(base, fix=pa.array([bytes([i % 256]) * 16 for i in range(n)], pa.binary(16))))
    p2 = put("flba", flba, compression="none")
    with pytest.raises(NotImplementedError, match="'fix'.*FIXED_LEN_BYTE_ARRAY"):
        read_parquet_columns(fs, p2, ["fix"], device=device)
    ts = pa.table(dict(base, ts=pa.array(np.arange(n) * 10 ** 9, pa.timestamp("ns"))))
    p3 = put("int96", ts, compression="none", use_deprecated_int96_timestamps=True)
    with pytest.raises(NotImplementedError, match="'ts'.*INT96"):
        read_parquet_columns(fs, p3, ["ts"], device=device)
    assert lib().parquet_decode_launches() == before   # all refused from the footer
    # unselected, such columns do not disturb the others (columns=None leaves them out)
    for path, tbl in ((p, nested), (p2, flba), (p3, ts)):
        ok(path, tbl)
        assert read_parquet_columns(fs, path, device=device).names == ["id", "name"]
    # an encoding that only the page headers reveal
    p4 = put("delta", pa.table(base), compression="none", use_dictionary=False, column_encoding={"id": "DELTA_BINARY_PACKED"})
    with pytest.raises(NotImplementedError, match="'id'.*DELTA_BINARY_PACKED"):
        read_parquet_columns(fs, p4, ["id"], device=device)
    # logical types are not interpreted: a timestamp is its int64
    p5 = put("ts", ts, compression="none")
    assert read_parquet_columns(fs, p5, ["ts"], device=device)["ts"].tolist() == (np.arange(n) * 10 ** 9).tolist()
    fs.close()


def _run_metadata(c):
    fs = c.client()
    for form in ("v1", "v2-lz4", "plain"):
        blob = _blob(form)
        fs.write_file(f"/pq/m-{form}.parquet", blob, write_type="MUST_CACHE")
        md = parquet_metadata(fs, f"/pq/m-{form}.parquet")
        ref = pq.ParquetFile(io.BytesIO(blob)).metadata
        assert md.num_rows == ref.num_rows and len(md.row_groups) == ref.num_row_groups and md.created_by == ref.created_by
        assert len(md.schema) == ref.num_columns
        for j, lf in enumerate(md.schema):
            col = ref.schema.column(j)
            assert (lf.name, lf.physical_type, lf.max_definition_level, lf.max_repetition_level) == \
                   (col.path, col.physical_type, col.max_definition_level, col.max_repetition_level)
            assert lf.repetition == ("REQUIRED" if lf.name == "seq" else "OPTIONAL")
        for g, rg in enumerate(md.row_groups):
            rr = ref.row_group(g)
            assert rg.num_rows == rr.num_rows and len(rg.columns) == rr.num_columns
            for j, cc in enumerate(rg.columns):
                rc = rr.column(j)
                codec = {"LZ4_RAW": "LZ4"}.get(cc.codec, cc.codec)        # pyarrow's name for codec 7
                assert (cc.name, cc.physical_type, codec, cc.num_values, cc.data_page_offset, cc.total_compressed_size) == \
                       (rc.path_in_schema, rc.physical_type, rc.compression, rc.num_values, rc.data_page_offset,
                        rc.total_compressed_size)
                assert cc.dictionary_page_offset == rc.dictionary_page_offset
                assert cc.codec == ("LZ4_RAW" if form == "v2-lz4" else "UNCOMPRESSED")
    # a nested schema: dotted leaf names and levels
    buf = io.BytesIO()
    pq.write_table(pa.table({"s": pa.array([{"a": 1, "b": [1.5]}, None], pa.struct([("a", pa.int32()), ("b", pa.list_(pa.float64()))]))}), buf)
    fs.write_file("/pq/m-nested.parquet", buf.getvalue(), write_type="MUST_CACHE")
    md = parquet_metadata(fs, "/pq/m-nested.parquet")
    ref = pq.ParquetFile(io.BytesIO(buf.getvalue())).metadata
    assert [(lf.name, lf.max_definition_level, lf.max_repetition_level) for lf in md.schema] == \
           [(ref.schema.column(j).path, ref.schema.column(j).max_definition_level, ref.schema.column(j).max_repetition_level)
            for j in range(ref.num_columns)]
    fs.close()


def _run_transform(c, device):
    """transformTable with parquet.compression=lz4 writes what read_parquet_columns reads."""
    from types import SimpleNamespace

    from alluxio_amd.job.plans import TransformDefinition
    fs = c.client()
    tbl = _table(n=400, seed=2)
    buf = io.BytesIO()
    pq.write_table(tbl, buf)                            # the default: snappy
    fs.create_directory("/pq/src", recursive=True, allow_exists=True)
    fs.write_file("/pq/src/part-0.parquet", buf.getvalue(), write_type="MUST_CACHE")
    plan = TransformDefinition()
    assert plan._write_options("file.count.max=2") == {} and plan._max_files("file.count.max=2;parquet.compression=lz4") == 2
    args = {"files": ["/pq/src/part-0.parquet"], "dst": "/pq/dst", "spec": "_"}
    out = plan.run_task(SimpleNamespace(transform="file.count.max=1;parquet.compression=lz4"), args, SimpleNamespace(fs=fs))
    (path,) = out["files"]
    assert {cc.codec for rg in parquet_metadata(fs, path).row_groups for cc in rg.columns} == {"LZ4_RAW"}
    _check(read_parquet_columns(fs, path, device=device), tbl)
    with pytest.raises(NotImplementedError, match="SNAPPY"):
        read_parquet_columns(fs, "/pq/src/part-0.parquet", device=device)
    fs.close()


@pytest.mark.parametrize("form", list(FORMS))
def test_parquet_forms_cpu(form):
    from alluxio_amd.ops.native import lib
    before = lib().parquet_decode_launches()
    with _cluster("dram") as c:
        _run_forms(c, "cpu", form)
    assert lib().parquet_decode_launches() == before   # the host loops


def test_parquet_interface_cpu():
    with _cluster("dram") as c:
        _run_interface(c, "cpu")


def test_parquet_refusals_cpu():
    with _cluster("dram") as c:
        _run_refusals(c, "cpu")


def test_parquet_metadata_cpu():
    with _cluster("dram") as c:
        _run_metadata(c)


def test_parquet_transform_cpu():
    with _cluster("dram") as c:
        _run_transform(c, "cpu")


@pytest.fixture(params=[pytest.param(0, id="gpu-v0"), pytest.param(1, id="gpu-v1")])
def variant(request, gpu):
    from alluxio_amd.ops.native import lib
    default = lib().parquet_decode_variant()
    lib().set_parquet_decode_variant(request.param)
    yield request.param
    lib().set_parquet_decode_variant(default)


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_parquet_forms(variant, form):
    from alluxio_amd.ops.native import lib
    before = lib().parquet_decode_launches()
    with _cluster("hbm:0") as c:
        _run_forms(c, "cuda", form)
    assert lib().parquet_decode_launches() > before    # the kernels


@pytest.mark.gpu
def test_parquet_interface(variant):
    with _cluster("hbm:0") as c:
        _run_interface(c, "cuda")


@pytest.mark.gpu
def test_parquet_refusals(variant):
    with _cluster("hbm:0") as c:
        _run_refusals(c, "cuda")


@pytest.mark.gpu
def test_parquet_transform(variant):
    with _cluster("hbm:0") as c:
        _run_transform(c, "cuda")
