"""parse_fields and read_delimited_columns: a CSV from csv.writer (quoted fields with commas, line
breaks and doubled quotes, numeric and string columns, a header) read back as typed columns and
compared with the values handed to the writer; loader batches in both layouts and both plans; a
TSV without a quote; deferred floats; the error paths.  CPU variants run on a DRAM-tier mini
cluster (the host loop), gpu variants on the HBM tier (the kernel)."""
import csv
import io

import numpy as np
import pytest

from alluxio_amd.minicluster import LocalAlluxioCluster
from alluxio_amd.models import (DeviceBatchLoader, FieldColumns, IndexedRecordDataset, RaggedBatch, parse_fields,
                                read_delimited_columns)

PIECES = ["a", "b", "c d", ",", '""', "\n", "\r\n", "x,y", 'say "hi"', "line one\nline two", " "]
HEADER = ["id", "score", "note", "count", "ratio", "tag"]
NROWS = 700


def _cluster(path):
    return LocalAlluxioCluster(num_workers=1, conf={"alluxio.worker.tieredstore.level0.dirs.path": path,
                                                    "alluxio.worker.hbm.page.size": "64KB",
                                                    "alluxio.user.block.size.bytes.default": "256KB"})


def _table():
    """Rows as handed to csv.writer: id int, score float (some outside the fast path), note text with
    commas, line breaks and quotes, count int or empty, ratio float text, tag text."""
    rng = np.random.default_rng(12)
    rows = []
    for r in range(NROWS):
        note = "".join(PIECES[i] for i in rng.integers(0, len(PIECES), int(rng.integers(0, 9))))
        score = [float(rng.integers(-10 ** 6, 10 ** 6)) / 64.0, float(rng.standard_normal()) * 1e30,
                 float(rng.random())][int(rng.integers(0, 3))]
        count = "" if r % 11 == 3 else int(rng.integers(-2 ** 31, 2 ** 31))
        ratio = ["0.5", "1e3", "-2.25", "nan", "7"][int(rng.integers(0, 5))]
        rows.append([r * 7919 - 10 ** 6, repr(score), note, count, ratio, f"t{r % 13}"])
    return rows


def _csv(rows, header=True, **kw):
    buf = io.StringIO()
    w = csv.writer(buf, lineterminator="\n", **kw)
    if header:
        w.writerow(HEADER)
    w.writerows(rows)
    return buf.getvalue().encode()


def _np(t):
    return t.cpu().numpy()


def _spans(blob, col):
    start, length = _np(col.start), _np(col.length)
    return [blob[s:s + n] for s, n in zip(start, length)]


def _check_table(got: FieldColumns, rows, blob, by_name):
    key = (lambda n, k: n) if by_name else (lambda n, k: k)
    ident, score, note, count = got[key("id", 0)], got[key("score", 1)], got[key("note", 2)], got[key("count", 3)]
    assert got.rows == len(rows)
    assert (_np(ident.status) == 0).all() and _np(ident.values).tolist() == [r[0] for r in rows]
    assert (_np(score.status) == 0).all()                # deferred ones were resolved
    want = np.array([float(r[1]) for r in rows])
    assert np.array_equal(_np(score.values).view(np.int64), want.view(np.int64))
    empty = np.array([r[3] == "" for r in rows])
    assert np.array_equal(_np(count.status), empty.astype(np.uint8))
    assert _np(count.values).tolist() == [0 if r[3] == "" else r[3] for r in rows] and _np(count.values).dtype == np.int32
    # the span, sliced out of the file, is the raw field: csv's quoting undone gives the text back
    assert (_np(note.status) == 0).all()
    for raw, r in zip(_spans(blob, note), rows):
        text = raw.decode().replace('""', '"')
        assert text == r[2].strip(" \t") or (raw == b"" and r[2].strip(" \t") == ""), (raw, r[2])


def _run(c, device):
    import torch
    fs = c.client()
    rows = _table()
    blob = _csv(rows)
    assert b'""' in blob and b',"' in blob
    fs.write_file("/t/table.csv", blob, write_type="MUST_CACHE")

    named = {"id": ("id", "int64"), "score": ("score", "float64"), "note": ("note", "span"), "count": ("count", "int32")}
    got = read_delimited_columns(fs, "/t/table.csv", named, quote='"', header=True, batch_size=256, device=device)
    assert got.names == list(named) and got["id"].values.device.type == torch.device(device).type
    _check_table(got, rows, blob, True)
    # by position: a list when the header is only skipped
    listed = [(0, "int64"), (1, "float64"), (2, "span"), (3, "int32")]
    got = read_delimited_columns(fs, "/t/table.csv", listed, quote='"', header=True, batch_size=100, device=device,
                                 device_plan=False)
    _check_table(got, rows, blob, False)
    same = read_delimited_columns(fs, "/t/table.csv", listed, quote='"', skip_rows=1, batch_size=65536, device=device)
    for a, b in zip(got, same):
        for x, y in zip(a._tensors(), b._tensors()):
            assert torch.equal(x, y)
    got = read_delimited_columns(fs, "/t/table.csv", named, quote='"', header=True, skip_rows=200, device=device)
    first = blob.index(b"\n" + str(rows[200][0]).encode() + b",") + 1
    _check_table(got, rows[200:], blob, True)
    assert int(got["note"].start[0]) > first
    none = read_delimited_columns(fs, "/t/table.csv", named, quote='"', header=True, skip_rows=10 ** 6, device=device)
    assert none.rows == 0 and none["score"].values.dtype == torch.float64

    # error paths
    with pytest.raises(KeyError):
        read_delimited_columns(fs, "/t/table.csv", {"x": ("nope", "int64")}, quote='"', header=True, device=device)
    fs.write_file("/t/dup.csv", b"a,b,a\n1,2,3\n", write_type="MUST_CACHE")
    with pytest.raises(ValueError, match="twice"):
        read_delimited_columns(fs, "/t/dup.csv", {"x": ("b", "int64")}, header=True, device=device)
    with pytest.raises(ValueError, match="header"):
        read_delimited_columns(fs, "/t/dup.csv", [("b", "int64")], device=device)
    with pytest.raises(ValueError, match="differ"):
        read_delimited_columns(fs, "/t/dup.csv", [(0, "int64")], quote=",", device=device)
    with pytest.raises(ValueError, match="unknown column type"):
        read_delimited_columns(fs, "/t/dup.csv", [(0, "complex")], device=device)

    # parse_fields on loader batches: packed and padded, planned and general path give the same columns
    ds = IndexedRecordDataset.from_delimited(fs, "/t/table.csv", quote='"', device=device)
    cols = {"id": (0, "int64"), "score": (1, "float64"), "note": (2, "span"), "ratio": (4, "float32"), "tag": (5, "span"),
            "gone": (6, "int64")}
    results = {}
    for layout, align in (("packed", 1), ("packed", 16), ("padded", 1)):
        for plan in ("auto", False):
            seen, parts = 1, []                          # record 0 is the header
            with DeviceBatchLoader(ds, batch_size=97, device=device, layout=layout, align=align, device_plan=plan) as dl:
                for bi, batch in enumerate(dl):
                    assert isinstance(batch, RaggedBatch) and batch.data.dim() == (2 if layout == "padded" else 1)
                    got = parse_fields(batch, cols, quote='"')
                    flat = _np(batch.data).reshape(-1)
                    lo = 1 if bi == 0 else 0
                    tags, notes = got["tag"], got["note"]
                    for j in range(lo, got.rows):
                        r = rows[seen - 1]
                        s, n = int(tags.start[j]), int(tags.length[j])
                        assert flat[s:s + n].tobytes().decode() == r[5]
                        s, n = int(notes.start[j]), int(notes.length[j])
                        assert flat[s:s + n].tobytes().decode().replace('""', '"') == r[2].strip(" \t")
                        seen += 1
                    if bi == 0:
                        assert int(got["id"].status[0]) == 2 and int(got["score"].status[0]) == 2      # the header's text
                    parts.append(got)
                assert (dl._gather is not None) == (plan == "auto")
            assert seen == NROWS + 1
            whole = FieldColumns.concat(parts)
            assert _np(whole["id"].values)[1:].tolist() == [r[0] for r in rows]
            want = np.array([np.float32(float(r[4])) for r in rows])
            gr = _np(whole["ratio"].values)[1:]
            assert np.array_equal(np.isnan(gr), np.isnan(want)) and np.array_equal(gr[~np.isnan(want)], want[~np.isnan(want)])
            assert (_np(whole["gone"].status) == 1).all() and (_np(whole["gone"].values) == 0).all()
            results[(layout, align, plan)] = whole
    base = results[("packed", 1, "auto")]
    for key, whole in results.items():
        for name in ("id", "score", "ratio", "gone"):
            a, b = base[name], whole[name]
            assert torch.equal(a.status, b.status), (key, name)
            assert torch.equal(a.values.view(torch.int32 if name == "ratio" else torch.int64),
                               b.values.view(torch.int32 if name == "ratio" else torch.int64)), (key, name)
        assert torch.equal(base["note"].length, whole["note"].length) and torch.equal(base["tag"].length, whole["tag"].length)

    # deferred floats stay NaN with status 3 on request
    with DeviceBatchLoader(ds, batch_size=NROWS + 1, device=device, align=1) as dl:
        (batch,) = list(dl)
    raw = parse_fields(batch, [(1, "float64")], quote='"', resolve_deferred=False)
    done = parse_fields(batch, [(1, "float64")], quote='"')
    st = _np(raw[0].status)[1:]
    assert set(st.tolist()) == {0, 3} and (st == 3).sum() > NROWS // 5
    assert np.isnan(_np(raw[0].values)[1:][st == 3]).all() and (_np(done[0].status)[1:] == 0).all()
    assert np.array_equal(_np(raw[0].values)[1:][st == 0], _np(done[0].values)[1:][st == 0])

    # a non-uint8 batch
    with pytest.raises(ValueError, match="uint8"):
        parse_fields(RaggedBatch(batch.data.to(torch.int16), batch.offsets, batch.lengths), [(0, "int64")])
    with pytest.raises(ValueError, match="at least one"):
        parse_fields(batch, [])

    # a TSV without a quote: quote bytes are ordinary text
    tsv_rows = [[i, f"{i / 8:.3f}", f'he said "{i}"', i * i] for i in range(300)]
    tsv = "".join("\t".join(str(x) for x in r) + "\r\n" for r in tsv_rows).encode()
    fs.write_file("/t/table.tsv", tsv, write_type="MUST_CACHE")
    got = read_delimited_columns(fs, "/t/table.tsv", [(0, "int32"), (1, "float64"), (2, "span"), (3, "int64")], sep="\t",
                                 batch_size=128, device=device)
    assert _np(got[0].values).tolist() == [r[0] for r in tsv_rows] and _np(got[3].values).tolist() == [r[3] for r in tsv_rows]
    assert _np(got[1].values).tolist() == [float(r[1]) for r in tsv_rows]
    assert [x.decode() for x in _spans(tsv, got[2])] == [r[2] for r in tsv_rows]
    for c in got:
        assert (_np(c.status) == 0).all()
    fs.close()


def test_field_columns_cpu():
    from alluxio_amd.ops.native import lib
    before = lib().field_parse_launches()
    with _cluster("dram") as c:
        _run(c, "cpu")
    assert lib().field_parse_launches() == before       # the host loop


@pytest.mark.gpu
def test_field_columns_gpu(gpu):
    from alluxio_amd.ops.native import lib
    before = lib().field_parse_launches()
    with _cluster("hbm:0") as c:
        _run(c, "cuda")
    assert lib().field_parse_launches() > before        # the kernel
