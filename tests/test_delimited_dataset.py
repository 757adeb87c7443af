"""Delimited text files as datasets: build_delimited_index (store form: kernels on an HBM dir, the
host loop on a DRAM dir; and the stream fallback) against bytes.splitlines, then
IndexedRecordDataset.from_delimited + a packed DeviceBatchLoader epoch reproducing every line."""
import numpy as np
import pytest

from alluxio_amd.minicluster import LocalAlluxioCluster
from alluxio_amd.models import (DeviceBatchLoader, IndexedRecordDataset, build_delimited_index, read_index)

BATCH = 8


def _cluster(path):
    return LocalAlluxioCluster(num_workers=1, conf={"alluxio.worker.tieredstore.level0.dirs.path": path,
                                                    "alluxio.worker.hbm.page.size": "64KB",
                                                    "alluxio.user.block.size.bytes.default": "256KB"})


def _write(fs):
    """Two text files of about 600 KB, line lengths in [0, 5000] with empty lines; the first ends
    without a newline, the second with one.  (paths, contents)."""
    rng = np.random.default_rng(33)
    paths, blobs = [], []
    for k in range(2):
        lines = []
        while sum(len(x) + 1 for x in lines) < 600_000:
            n = 0 if rng.random() < 0.05 else int(rng.integers(0, 5001))
            body = rng.integers(0, 256, n, dtype=np.uint8)
            body[(body == 0x0A) | (body == 0x0D)] = 0x20     # '\n' only ends a line, and no '\r' for splitlines
            lines.append(body.tobytes())
        assert b"" in lines
        blob = b"\n".join(lines) + (b"\n" if k == 1 else b"x")
        p = f"/txt/part-{k}.jsonl"
        fs.write_file(p, blob, write_type="MUST_CACHE")
        paths.append(p)
        blobs.append(blob)
    assert not blobs[0].endswith(b"\n") and blobs[1].endswith(b"\n")
    return paths, blobs


def _no_stream(fs):
    """Make fs.open_file fail: what runs meanwhile did not read the file through the client."""
    real = fs.open_file

    def forbidden(*a, **kw):
        raise AssertionError("the file was read through the client stream")

    fs.open_file = forbidden
    return real


def _check(c, device):
    fs = c.client()
    worker = c.workers[0].worker
    paths, blobs = _write(fs)
    flat = []
    for p, blob in zip(paths, blobs):
        lines = blob.splitlines(keepends=True)
        want = np.concatenate([[0], np.cumsum([len(x) for x in lines])]).astype(np.int64)
        real = _no_stream(fs)
        try:
            off = build_delimited_index(fs, p)          # in-process worker, one memory dir: the store form
        finally:
            fs.open_file = real
        assert off.dtype == np.int64 and np.array_equal(off, want)
        assert np.array_equal(build_delimited_index(fs, p, device_plan=False, chunk_bytes=100_003), want)
        assert np.array_equal(build_delimited_index(fs, p, b"\n", write=True, write_type="MUST_CACHE"), want)
        assert np.array_equal(read_index(fs, p), want)
        flat += lines
    assert int(want[-1]) == len(blobs[1])

    ds = IndexedRecordDataset.from_delimited(fs, paths, device=device)
    assert len(ds) == len(flat) and np.array_equal(ds.lengths, [len(x) for x in flat])
    seen = 0
    with DeviceBatchLoader(ds, batch_size=BATCH, device=device, align=1) as dl:
        for data, off, ln in dl:
            data, off, ln = data.cpu().numpy(), off.cpu().numpy(), ln.cpu().numpy()
            for r in range(len(ln)):
                assert data[off[r]:off[r] + ln[r]].tobytes() == flat[seen], seen
                seen += 1
        assert dl._gather is not None                   # the fast loader path took the built index
    assert seen == len(flat)
    fs.delete(paths[1] + ".idx")
    one = IndexedRecordDataset.from_delimited(fs, paths[1], write_index=True)
    assert len(one) == len(blobs[1].splitlines()) and np.array_equal(read_index(fs, paths[1]), one.offsets[0])

    # another delimiter, and an empty file
    comma = build_delimited_index(fs, paths[0], ",")
    raw = np.frombuffer(blobs[0], dtype=np.uint8)
    cuts = np.flatnonzero(raw == ord(",")) + 1
    assert cuts.size > 100 and np.array_equal(comma, np.concatenate([[0], cuts, [len(raw)]]))
    fs.write_file("/txt/empty", b"", write_type="MUST_CACHE")
    assert build_delimited_index(fs, "/txt/empty").tolist() == [0]
    assert build_delimited_index(fs, "/txt/empty", device_plan=False).tolist() == [0]
    assert len(IndexedRecordDataset.from_delimited(fs, "/txt/empty")) == 0
    for bad in (b"\r\n", b"", "ab"):
        with pytest.raises(ValueError, match="one byte"):
            build_delimited_index(fs, paths[0], bad)
    with pytest.raises(ValueError, match="one byte"):
        IndexedRecordDataset.from_delimited(fs, paths, delimiter=b"\r\n")

    # nothing is left read-locked: the files can be deleted
    for p in paths:
        st = fs.get_status(p)
        for bid in st.info.blockIds:
            assert worker.native.block_info(bid).readers == 0
        fs.delete(p)
        assert not fs.exists(p)
    fs.close()


def test_delimited_dataset_cpu():
    with _cluster("dram") as c:
        _check(c, "cpu")


@pytest.mark.gpu
def test_delimited_dataset_gpu(gpu):
    from alluxio_amd.ops.native import lib
    before = lib().delim_index_launches()
    with _cluster("hbm:0") as c:
        _check(c, "cuda")
    assert lib().delim_index_launches() > before        # the index came from the kernels
