"""CSV files with line breaks inside quoted fields as datasets: build_delimited_index(quote='"')
(store form: kernels on an HBM dir, the host loop on a DRAM dir; and the stream fallback) against
the quote-parity rule in numpy and against csv.reader, then IndexedRecordDataset.from_delimited +
a packed DeviceBatchLoader epoch reproducing every row."""
import csv
import io

import numpy as np
import pytest

from alluxio_amd.minicluster import LocalAlluxioCluster
from alluxio_amd.models import (DeviceBatchLoader, IndexedRecordDataset, build_delimited_index, read_index)

BATCH = 8
PIECES = ["a", "b", "c d", ",", '"', '""', "\n", "\r\n", "x,y", 'say "hi"', "line one\nline two", ""]


def _cluster(path):
    return LocalAlluxioCluster(num_workers=1, conf={"alluxio.worker.tieredstore.level0.dirs.path": path,
                                                    "alluxio.worker.hbm.page.size": "64KB",
                                                    "alluxio.user.block.size.bytes.default": "256KB"})


def _rule(blob):
    """The offsets by the rule: a newline is a cut when an even number of quote bytes precedes it."""
    x = np.frombuffer(blob, dtype=np.uint8)
    q = x == ord('"')
    before = np.cumsum(q) - q
    cuts = np.flatnonzero((x == 0x0A) & (before % 2 == 0)) + 1
    off = np.concatenate([[0], cuts, [len(x)]]).astype(np.int64)
    return off[:-1] if cuts.size and cuts[-1] == len(x) else off


def _write(fs):
    """Two CSV files of about 600 KB from csv.writer: the fields hold commas, quotes, \\n and \\r\\n
    and are up to a few KB long, so quoted fields cross pages and blocks.  The first file ends
    without a newline, the second with one.  (paths, contents, rows per file)."""
    rng = np.random.default_rng(44)
    paths, blobs, tables = [], [], []
    for k in range(2):
        rows, size = [], 0
        while size < 600_000:
            row = []
            for _ in range(int(rng.integers(1, 6))):
                n = int(rng.integers(0, 12)) if rng.random() < 0.8 else int(rng.integers(200, 1500))
                row.append("".join(PIECES[i] for i in rng.integers(0, len(PIECES), n)))
            if row == [""]:
                row = ["", ""]                          # csv.writer writes a lone empty field as ""
            rows.append(row)
            size += sum(len(f) + 3 for f in row)
        buf = io.StringIO()
        csv.writer(buf, lineterminator="\n").writerows(rows)
        blob = buf.getvalue().encode()
        if k == 0:
            blob = blob[:-1]
        p = f"/csv/part-{k}.csv"
        fs.write_file(p, blob, write_type="MUST_CACHE")
        paths.append(p)
        blobs.append(blob)
        tables.append(rows)
    assert not blobs[0].endswith(b"\n") and blobs[1].endswith(b"\n")
    return paths, blobs, tables


def _no_stream(fs):
    """Make fs.open_file fail: what runs meanwhile did not read the file through the client."""
    real = fs.open_file

    def forbidden(*a, **kw):
        raise AssertionError("the file was read through the client stream")

    fs.open_file = forbidden
    return real


def _parse(record: bytes):
    got = list(csv.reader(io.StringIO(record.decode(), newline="")))
    assert len(got) == 1, record[:80]
    return got[0]


def _check(c, device):
    fs = c.client()
    worker = c.workers[0].worker
    paths, blobs, tables = _write(fs)
    flat_rows, flat = [], []
    for p, blob, rows in zip(paths, blobs, tables):
        want = _rule(blob)
        assert len(want) - 1 == len(rows)               # one record per row ...
        records = [blob[want[i]:want[i + 1]] for i in range(len(rows))]
        for rec, row in zip(records, rows):             # ... and each parses to its row
            assert _parse(rec) == row
        quotes_before = np.cumsum(np.frombuffer(blob, dtype=np.uint8) == ord('"'))
        edges = np.arange(64 << 10, len(blob), 64 << 10)
        assert (quotes_before[edges - 1] % 2 == 1).any()        # a page starts inside a quoted field
        assert not np.isin(edges[3::4], want).all()             # a block starts inside a record
        real = _no_stream(fs)
        try:
            off = build_delimited_index(fs, p, quote='"')       # in-process worker, one memory dir: the store form
        finally:
            fs.open_file = real
        assert off.dtype == np.int64 and np.array_equal(off, want)
        assert np.array_equal(build_delimited_index(fs, p, quote=b'"', device_plan=False, chunk_bytes=100_003), want)
        assert np.array_equal(build_delimited_index(fs, p, b"\n", '"', write=True, write_type="MUST_CACHE"), want)
        assert np.array_equal(read_index(fs, p), want)
        plain = build_delimited_index(fs, p, quote=None)        # unchanged: every newline cuts
        assert np.array_equal(plain, build_delimited_index(fs, p)) and len(plain) - 1 > len(rows)
        assert len(plain) - 1 == len(blob.split(b"\n")) - (1 if blob.endswith(b"\n") else 0)
        flat_rows += rows
        flat += records

    ds = IndexedRecordDataset.from_delimited(fs, paths, device=device, quote='"')
    assert len(ds) == len(flat) and np.array_equal(ds.lengths, [len(x) for x in flat])
    seen = 0
    with DeviceBatchLoader(ds, batch_size=BATCH, device=device, align=1) as dl:
        for data, off, ln in dl:
            data, off, ln = data.cpu().numpy(), off.cpu().numpy(), ln.cpu().numpy()
            for r in range(len(ln)):
                rec = data[off[r]:off[r] + ln[r]].tobytes()
                assert rec == flat[seen] and _parse(rec) == flat_rows[seen], seen
                seen += 1
        assert dl._gather is not None                   # the fast loader path took the built index
    assert seen == len(flat)
    assert len(IndexedRecordDataset.from_delimited(fs, paths)) > len(flat)

    # a file that ends inside quotes: its tail is the last record; and an empty file
    fs.write_file("/csv/open", b'a,b\n"c\nd\n', write_type="MUST_CACHE")
    assert build_delimited_index(fs, "/csv/open", quote='"').tolist() == [0, 4, 9]
    assert build_delimited_index(fs, "/csv/open", quote='"', device_plan=False, chunk_bytes=3).tolist() == [0, 4, 9]
    fs.write_file("/csv/empty", b"", write_type="MUST_CACHE")
    assert build_delimited_index(fs, "/csv/empty", quote='"').tolist() == [0]
    assert build_delimited_index(fs, "/csv/empty", quote='"', device_plan=False).tolist() == [0]
    for bad in ('""', b"", b"ab"):
        with pytest.raises(ValueError, match="one byte"):
            build_delimited_index(fs, paths[0], quote=bad)
    with pytest.raises(ValueError, match="differ"):
        build_delimited_index(fs, paths[0], ",", quote=",")
    with pytest.raises(ValueError, match="differ"):
        IndexedRecordDataset.from_delimited(fs, paths, quote=b"\n")
    with pytest.raises(ValueError, match="one byte"):
        IndexedRecordDataset.from_delimited(fs, paths, quote='""')

    # nothing is left read-locked: the files can be deleted
    for p in paths:
        st = fs.get_status(p)
        for bid in st.info.blockIds:
            assert worker.native.block_info(bid).readers == 0
        fs.delete(p)
        assert not fs.exists(p)
    fs.close()


def test_delimited_dataset_quoted_cpu():
    with _cluster("dram") as c:
        _check(c, "cpu")


@pytest.mark.gpu
def test_delimited_dataset_quoted_gpu(gpu):
    from alluxio_amd.ops.native import lib
    before = lib().delim_index_launches()
    with _cluster("hbm:0") as c:
        _check(c, "cuda")
    assert lib().delim_index_launches() > before        # the index came from the kernels
