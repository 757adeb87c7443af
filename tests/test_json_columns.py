"""parse_json_fields, unescape_json_text and read_json_columns: a JSON Lines file from json.dumps
(an int, floats some of which lie outside the fast path, a bool, a nullable field, a text with line
breaks, quotes and emoji, a label with 13 distinct values) read back as typed columns and compared
with the Python objects that were dumped; loader batches in both layouts; 33 columns; a dictionary
shared by two files; deferred floats; the error paths; an empty file.  CPU variants run on a
DRAM-tier mini cluster (the host loops), gpu variants on the HBM tier (the kernels)."""
import json

import numpy as np
import pytest

from alluxio_amd.minicluster import LocalAlluxioCluster
from alluxio_amd.models import (DeviceBatchLoader, FieldColumns, IndexedRecordDataset, TextDictionary, parse_json_fields,
                                read_json_columns, unescape_json_text)

PIECES = ["a", "b", "c d", ",", '"', "\n", "\r\n", "\\", "{x}", "é", "\U0001f600", "line one\nline two", " ", "\t"]
NROWS = 700


def _cluster(path):
    return LocalAlluxioCluster(num_workers=1, conf={"alluxio.worker.tieredstore.level0.dirs.path": path,
                                                    "alluxio.worker.hbm.page.size": "64KB",
                                                    "alluxio.user.block.size.bytes.default": "256KB"})


def _objects(seed=12, n=NROWS):
    rng = np.random.default_rng(seed)
    objs = []
    for r in range(n):
        text = "".join(PIECES[i] for i in rng.integers(0, len(PIECES), int(rng.integers(0, 9))))
        score = [float(rng.integers(-10 ** 6, 10 ** 6)) / 64.0, float(rng.standard_normal()) * 1e30,
                 float(rng.random())][int(rng.integers(0, 3))]
        o = {"id": r * 7919 - 10 ** 6, "score": score, "ok": bool(rng.integers(0, 2)),
             "count": None if r % 11 == 3 else int(rng.integers(-2 ** 31, 2 ** 31)), "text": text,
             "label": f"t{(r * 5 + seed) % 13}", "meta": {"id": -1, "tags": ["x", {"label": "no"}]}}
        if r % 7 == 2:
            del o["count"]                              # absent and null both read as "no value"
        objs.append(o)
    return objs


def _jsonl(objs):
    return "".join(json.dumps(o, ensure_ascii=bool(i % 2), separators=(",", ":") if i % 3 else None) + "\n"
                   for i, o in enumerate(objs)).encode()


def _np(t):
    return t.cpu().numpy()


COLS = {"id": ("id", "int64"), "score": ("score", "float64"), "ok": ("ok", "bool"), "count": ("count", "int32"),
        "text": ("text", "text"), "label": ("label", "category"), "meta": ("meta", "span"), "ratio": ("score", "float32")}


def _check(got: FieldColumns, objs, blob=None):
    import torch
    assert got.rows == len(objs) and got.names == list(COLS)
    assert (_np(got["id"].status) == 0).all() and _np(got["id"].values).tolist() == [o["id"] for o in objs]
    assert (_np(got["score"].status) == 0).all()        # deferred ones were resolved
    want = np.array([o["score"] for o in objs], dtype=np.float64)
    assert np.array_equal(_np(got["score"].values).view(np.int64), want.view(np.int64))
    with np.errstate(over="ignore"):
        assert np.array_equal(_np(got["ratio"].values).view(np.int32), want.astype(np.float32).view(np.int32))
    assert got["ok"].values.dtype == torch.bool and got["ok"].tolist() == [o["ok"] for o in objs]
    assert got["count"].tolist() == [o.get("count") for o in objs] and got["count"].values.dtype == torch.int32
    assert set(_np(got["count"].status).tolist()) <= {0, 1}
    assert got["text"].tolist() == [o["text"].encode() for o in objs]
    assert _np(got["text"].length).tolist() == [len(o["text"].encode()) for o in objs]
    vocab = got["label"].dictionary.tolist()
    assert [vocab[c] for c in _np(got["label"].values)] == [o["label"].encode() for o in objs]
    if blob is not None:                                # span starts are file offsets
        for (s, n), o in zip(got["meta"].tolist(), objs):
            assert json.loads(blob[s:s + n]) == o["meta"]


def _run(c, device):
    import torch
    fs = c.client()
    objs = _objects()
    blob = _jsonl(objs)
    assert b"\\n" in blob and b'\\"' in blob and b"\\ud83d\\ude00" in blob and "\U0001f600".encode() in blob
    fs.write_file("/j/a.jsonl", blob, write_type="MUST_CACHE")
    got = read_json_columns(fs, "/j/a.jsonl", COLS, batch_size=256, device=device)
    assert got["id"].values.device.type == torch.device(device).type
    _check(got, objs, blob)
    assert len(got["label"].dictionary) == 13
    same = read_json_columns(fs, "/j/a.jsonl", COLS, batch_size=65536, device=device, device_plan=False)
    for a, b in zip(got, same):
        if a.type != got["label"].type:
            for x, y in zip(a._tensors(), b._tensors()):
                assert torch.equal(x, y)
    _check(read_json_columns(fs, "/j/a.jsonl", COLS, skip_rows=200, batch_size=100, device=device), objs[200:], blob)
    none = read_json_columns(fs, "/j/a.jsonl", COLS, skip_rows=10 ** 6, device=device)
    assert none.rows == 0 and none["score"].values.dtype == torch.float64 and none["ok"].values.dtype == torch.bool
    # a list of columns; one dictionary shared by two files
    objs2 = _objects(seed=5, n=90)
    fs.write_file("/j/b.jsonl", _jsonl(objs2), write_type="MUST_CACHE")
    d = TextDictionary(device)
    one = read_json_columns(fs, "/j/a.jsonl", [("label", "category"), ("id", "int32")], device=device, dictionaries={0: d})
    two = read_json_columns(fs, "/j/b.jsonl", [("label", "category"), ("id", "int32")], device=device, dictionaries={0: d})
    assert one[0].dictionary is d and two[0].dictionary is d and len(d) == 13
    vocab = d.tolist()
    assert [vocab[c] for c in _np(two[0].values)] == [o["label"].encode() for o in objs2]
    both = FieldColumns.concat([one, two])
    assert both.rows == NROWS + 90 and [vocab[c] for c in _np(both[0].values)][NROWS:] == [o["label"].encode() for o in objs2]
    # an empty file, and a file of blank and bad rows
    fs.write_file("/j/empty.jsonl", b"", write_type="MUST_CACHE")
    got = read_json_columns(fs, "/j/empty.jsonl", COLS, device=device)
    assert got.rows == 0 and got["text"].data.numel() == 0 and got["text"].offsets.tolist() == [0]
    fs.write_file("/j/odd.jsonl", b'\n{"id":1,"text":"a\\qb"}\r\n[1]\n{"id":2,"text":""}\n{"id":3,"text":null}\n{"id":4',
                  write_type="MUST_CACHE")
    got = read_json_columns(fs, "/j/odd.jsonl", {"id": ("id", "int64"), "text": ("text", "text")}, device=device)
    assert _np(got["id"].status).tolist() == [1, 0, 2, 0, 0, 2] and got["id"].tolist() == [None, 1, None, 2, 3, None]
    assert _np(got["text"].status).tolist() == [1, 2, 2, 0, 1, 2] and got["text"].tolist() == [None, None, None, b"", None, None]

    # parse_json_fields on loader batches: packed and padded give the same columns; 33 columns
    ds = IndexedRecordDataset.from_delimited(fs, "/j/a.jsonl", device=device)
    wide = {f"c{j}": (["id", "score", "ok", "count", "label"][j % 5], ["int64", "float64", "bool", "int32", "text"][j % 5])
            for j in range(33)}
    results = {}
    for layout, align in (("packed", 1), ("packed", 16), ("padded", 1)):
        parts, wides = [], []
        with DeviceBatchLoader(ds, batch_size=97, device=device, layout=layout, align=align) as dl:
            for batch in dl:
                assert batch.data.dim() == (2 if layout == "padded" else 1)
                parts.append(parse_json_fields(batch, COLS, dictionaries={"label": results.get("dict")}
                                               if "dict" in results else None))
                results.setdefault("dict", parts[-1]["label"].dictionary)
                wides.append(parse_json_fields(batch, wide))
        whole = FieldColumns.concat(parts)
        _check(whole, objs)
        w = FieldColumns.concat(wides)
        assert len(w) == 33 and w["c30"].tolist() == [o["id"] for o in objs] and w["c32"].tolist() == [o["ok"] for o in objs]
        assert w["c29"].tolist() == [o["label"].encode() for o in objs] and w["c31"].tolist() == [o["score"] for o in objs]
        results[(layout, align)] = whole
    base = results[("packed", 1)]
    for key in (("packed", 16), ("padded", 1)):
        for name in ("id", "score", "ok", "count", "label", "ratio"):
            assert torch.equal(base[name].status, results[key][name].status)
            assert torch.equal(base[name].values.view(torch.uint8), results[key][name].values.view(torch.uint8)), (key, name)
        assert torch.equal(base["text"].data, results[key]["text"].data)

    # deferred floats stay NaN with status 3 on request
    with DeviceBatchLoader(ds, batch_size=NROWS, device=device, align=1) as dl:
        (batch,) = list(dl)
    raw = parse_json_fields(batch, [("score", "float64")], resolve_deferred=False)
    done = parse_json_fields(batch, [("score", "float64")])
    st = _np(raw[0].status)
    assert set(st.tolist()) == {0, 3} and (st == 3).sum() > NROWS // 5
    assert np.isnan(_np(raw[0].values)[st == 3]).all() and (_np(done[0].status) == 0).all()
    assert np.array_equal(_np(raw[0].values)[st == 0], _np(done[0].values)[st == 0])

    # unescape_json_text on the spans of a string located as a span (with its quotes)
    spans = parse_json_fields(batch, [("text", "span")])[0]
    text, status = unescape_json_text(batch.data, spans.start + 1, spans.length - 2, spans.status)
    cuts, packed = _np(text.offsets), _np(text.data).tobytes()
    assert (_np(status) == 0).all() and [packed[cuts[r]:cuts[r + 1]] for r in range(NROWS)] == [o["text"].encode() for o in objs]
    text, status = unescape_json_text(torch.from_numpy(np.frombuffer(b"a\\tb\\qc\\u00e9", dtype=np.uint8).copy()).to(device),
                                      [0, 4, 7, 20], [4, 3, 6, 1], [0, 0, 0, 0])
    assert _np(status).tolist() == [0, 2, 0, 2] and _np(text.lengths).tolist() == [3, 0, 2, 0] and _np(text.data).tobytes() == b"a\tb\xc3\xa9"

    # error paths
    for key in ('a"b', "a\\b", "a\nb", "", "k" * 256):
        with pytest.raises(ValueError, match="key"):
            parse_json_fields(batch, [(key, "int64")])
    with pytest.raises(TypeError):
        parse_json_fields(batch, [(0, "int64")])
    with pytest.raises(ValueError, match="unknown column type"):
        read_json_columns(fs, "/j/a.jsonl", [("id", "complex")], device=device)
    with pytest.raises(ValueError, match="at least one"):
        parse_json_fields(batch, [])
    with pytest.raises(ValueError, match="uint8"):
        parse_json_fields(type(batch)(batch.data.to(torch.int16), batch.offsets, batch.lengths), [("id", "int64")])
    assert "bool" in repr(done[0].__class__("ok", "ok", 7, raw[0].status, None, raw[0].status))
    fs.close()


def test_json_columns_cpu():
    from alluxio_amd.ops.native import lib
    before = lib().json_fields_launches(), lib().json_text_launches()
    with _cluster("dram") as c:
        _run(c, "cpu")
    assert (lib().json_fields_launches(), lib().json_text_launches()) == before       # the host loops


@pytest.mark.gpu
def test_json_columns_gpu(gpu):
    from alluxio_amd.ops.native import lib
    before = lib().json_fields_launches(), lib().json_text_launches()
    with _cluster("hbm:0") as c:
        _run(c, "cuda")
    assert lib().json_fields_launches() > before[0] and lib().json_text_launches() > before[1]    # the kernels
