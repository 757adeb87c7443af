"""Variable-length record datasets: IndexedRecordDataset + DeviceBatchLoader yielding RaggedBatch
(CPU: DRAM tier + host tensors through the session's host loop; GPU: HBM tier + device tensors
through the plan + copy kernels), every batch compared with numpy slices of the written bytes."""
import numpy as np
import pytest

from alluxio_amd.minicluster import LocalAlluxioCluster
from alluxio_amd.models import (DeviceBatchLoader, FixedRecordDataset, IndexedRecordDataset, RaggedBatch,
                                read_index, write_index)

BATCH = 8


def _cluster(path):
    return LocalAlluxioCluster(num_workers=1, conf={"alluxio.worker.tieredstore.level0.dirs.path": path,
                                                    "alluxio.worker.hbm.page.size": "64KB",
                                                    "alluxio.user.block.size.bytes.default": "256KB"})


def _write(fs):
    """Two files of about 600 KB of records with lengths in [0, 70000]: (paths, offsets, records)."""
    rng = np.random.default_rng(21)
    paths, offsets, flat = [], [], []
    for k in range(2):
        lens = []
        while sum(lens) < 600_000 - 70_000:
            lens.append(int(rng.integers(0, 70_001)))
        lens[3] = 0
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        d = rng.integers(0, 256, int(off[-1]) + 123 * k, dtype=np.uint8)   # unindexed bytes after the last record
        fs.write_file(f"/rag/part-{k}", d, write_type="MUST_CACHE")
        paths.append(f"/rag/part-{k}")
        offsets.append(off)
        flat += [d[off[i]:off[i + 1]] for i in range(len(lens))]
    return paths, offsets, flat


def _check_batches(dl, flat, order, layout, align=16, max_len=None, pad=0, device_type="cpu"):
    seen, batches = 0, []
    for b, batch in enumerate(dl):
        assert isinstance(batch, RaggedBatch) and batch.data.device.type == device_type
        assert batch.offsets.device.type == device_type and batch.lengths.device.type == device_type
        idx = order[b * BATCH:(b + 1) * BATCH]
        data, off, ln = (t.cpu().numpy() for t in batch)
        assert off.dtype == np.int64 and off.shape == (len(idx) + 1,) and ln.shape == (len(idx),)
        if layout == "packed":
            want_len = np.array([len(flat[i]) for i in idx])
            adv = (want_len + align - 1) // align * align
            want_off = np.concatenate([[0], np.cumsum(adv)])
            want = np.zeros(int(want_off[-1]), dtype=np.uint8)
            for r, i in enumerate(idx):
                want[want_off[r]:want_off[r] + len(flat[i])] = flat[i]
            assert data.ndim == 1
        else:
            want_len = np.array([min(len(flat[i]), max_len) for i in idx])
            want_off = np.arange(len(idx) + 1) * max_len
            want = np.full((len(idx), max_len), pad, dtype=np.uint8)
            for r, i in enumerate(idx):
                want[r, :want_len[r]] = flat[i][:max_len]
            assert data.shape == (len(idx), max_len)
        assert np.array_equal(off, want_off) and np.array_equal(ln, want_len)
        assert np.array_equal(data, want)
        seen += len(idx)
        batches.append((data, off, ln))
    assert seen == len(flat) and len(dl) == -(-len(flat) // BATCH)
    assert len(flat) % BATCH != 0                       # the last batch was short
    return batches


def _check(c, device):
    import torch
    dev_type = torch.device(device).type
    fs = c.client()
    paths, offsets, flat = _write(fs)
    ds = IndexedRecordDataset(fs, paths, index=offsets, device=device)
    assert len(ds) == len(flat) and ds.locate(len(offsets[0]) - 1 + 2) == (1, int(offsets[1][2]))
    assert np.array_equal(ds.lengths, [len(r) for r in flat])
    for i in (0, 3, 5, len(offsets[0]) - 2, len(flat) - 1, -1):
        got = ds[i]
        assert got.ndim == 1 and got.device.type == dev_type and np.array_equal(got.cpu().numpy(), flat[i])
    order = np.random.default_rng(4).permutation(len(ds))
    worker = c.workers[0].worker
    bid = ds.files[0].block_ids[0]
    reads0 = worker.metrics.counter("BytesReadAlluxio").count

    with DeviceBatchLoader(ds, batch_size=BATCH, shuffle=True, seed=4, device=device) as dl:
        planned = _check_batches(dl, flat, order, "packed", device_type=dev_type)
        assert dl._gather is not None and dl._gather.gathers == len(dl)      # the session path ran
        assert worker.native.block_info(bid).readers > 0
    assert dl._gather is False
    # the gathered record bytes are counted in the worker's read metrics
    assert worker.metrics.counter("BytesReadAlluxio").count - reads0 == sum(len(r) for r in flat)
    with DeviceBatchLoader(ds, batch_size=BATCH, shuffle=True, seed=4, device=device, device_plan=False) as dl:
        general = _check_batches(dl, flat, order, "packed", device_type=dev_type)
        assert dl._gather is None
    for a, b in zip(planned, general):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))

    kw = dict(layout="padded", max_len=30_001, pad_value=0x5A)
    with DeviceBatchLoader(ds, batch_size=BATCH, shuffle=True, seed=4, device=device, **kw) as dl:
        planned = _check_batches(dl, flat, order, "padded", max_len=30_001, pad=0x5A, device_type=dev_type)
        assert dl._gather is not None and dl._gather.gathers == len(dl)
    with DeviceBatchLoader(ds, batch_size=BATCH, shuffle=True, seed=4, device=device, device_plan=False, **kw) as dl:
        general = _check_batches(dl, flat, order, "padded", max_len=30_001, pad=0x5A, device_type=dev_type)
    for a, b in zip(planned, general):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))

    # two-byte elements: offsets and lengths count elements
    even = [np.concatenate([[0], np.cumsum(np.diff(o) // 2 * 2)]).astype(np.int64) for o in offsets]
    ds16 = IndexedRecordDataset(fs, paths, index=even, dtype="int16", device=device)
    with DeviceBatchLoader(ds16, batch_size=BATCH, device=device, align=2) as dl:
        data, off, ln = (t.cpu().numpy() for t in next(iter(dl)))
        assert data.dtype == np.int16 and np.array_equal(ln, np.diff(even[0])[:BATCH] // 2)
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(ln)]))
        raw = fs.read_file(paths[0])
        assert data.tobytes() == raw[:int(even[0][BATCH])]
    with pytest.raises(ValueError):
        IndexedRecordDataset(fs, paths, index=offsets, dtype="int16")        # odd record lengths

    # after close() nothing is locked: the file can be deleted
    assert worker.native.block_info(bid).readers == 0
    fs.delete(paths[0])
    assert not fs.exists(paths[0])
    fs.close()


def test_ragged_loader_cpu():
    with _cluster("dram") as c:
        _check(c, "cpu")


@pytest.mark.gpu
def test_ragged_loader_gpu(gpu):
    with _cluster("hbm:0") as c:
        _check(c, "cuda")


def test_index_sidecar_round_trip():
    with _cluster("dram") as c:
        fs = c.client()
        paths, offsets, flat = _write(fs)
        for p, off in zip(paths, offsets):
            assert write_index(fs, p, off, write_type="MUST_CACHE") == p + ".idx"
            assert np.array_equal(read_index(fs, p), off)
        raw = fs.read_file(paths[0] + ".idx")
        assert raw[:8] == b"AMDXIDX1" and int.from_bytes(raw[8:16], "little") == len(offsets[0]) - 1
        assert len(raw) == 16 + 8 * len(offsets[0])
        ds = IndexedRecordDataset(fs, paths)                       # index=None: the sidecars
        assert len(ds) == len(flat)
        assert np.array_equal(ds[7].numpy(), flat[7]) and np.array_equal(ds[len(flat) - 2].numpy(), flat[-2])

        fs.write_file("/rag/badmagic.idx", b"AMDXIDX2" + raw[8:], write_type="MUST_CACHE")
        with pytest.raises(ValueError, match="magic"):
            read_index(fs, "/rag/badmagic")
        fs.write_file("/rag/short.idx", raw[:-8], write_type="MUST_CACHE")
        with pytest.raises(ValueError, match="truncated"):
            read_index(fs, "/rag/short")
        swapped = np.frombuffer(raw, dtype="<u8", offset=16).copy()
        swapped[[4, 5]] = swapped[[5, 4]]
        assert swapped[4] > swapped[5]
        fs.write_file("/rag/nonmono.idx", raw[:16] + swapped.tobytes(), write_type="MUST_CACHE")
        with pytest.raises(ValueError, match="decrease"):
            read_index(fs, "/rag/nonmono")
        with pytest.raises(ValueError, match="decrease"):
            write_index(fs, "/rag/x", [0, 10, 5])
        with pytest.raises(ValueError, match="past the end"):
            IndexedRecordDataset(fs, paths[0], index=np.append(offsets[0], offsets[0][-1] + 10 ** 6))
        fs.close()


def test_from_files_true_lengths_one_listing():
    with LocalAlluxioCluster(num_workers=1, conf={"alluxio.worker.tieredstore.level0.dirs.path": "dram",
                                                   "alluxio.user.block.size.bytes.default": "1MB"}) as c:
        fs = c.client()
        rng = np.random.default_rng(0)
        files = {}
        for i in range(40):
            n = [4096, 1000, 0, 70_001, 12_345][i % 5]
            files[i] = rng.integers(0, 256, n, dtype=np.uint8)
            fs.write_file(f"/img/{i:05d}", files[i], write_type="MUST_CACHE")
        calls = {"columns": 0, "other": 0}
        real_cols = fs.list_status_columns

        def counting_cols(*a, **kw):
            calls["columns"] += 1
            return real_cols(*a, **kw)

        def forbidden(*a, **kw):
            calls["other"] += 1
            raise AssertionError("per-file metadata call")

        fs.list_status_columns = counting_cols
        real_status, real_list = fs.get_status, fs.list_status
        fs.get_status = fs.list_status = forbidden
        try:
            ds = IndexedRecordDataset.from_files(fs, "/img")
        finally:
            fs.get_status, fs.list_status = real_status, real_list
        assert calls == {"columns": 1, "other": 0}
        assert len(ds) == 40 and np.array_equal(ds.lengths, [len(files[i]) for i in range(40)])
        seen = 0
        with DeviceBatchLoader(ds, batch_size=16, shuffle=True, seed=3, device="cpu", align=1) as dl:
            order = np.random.default_rng(3).permutation(40)
            for b, (data, off, ln) in enumerate(dl):
                for r in range(len(ln)):
                    i = int(order[b * 16 + r])
                    assert int(ln[r]) == len(files[i])               # nothing truncated
                    assert np.array_equal(data[int(off[r]):int(off[r]) + int(ln[r])].numpy(), files[i])
                    seen += 1
            assert dl._gather is not None
        assert seen == 40
        fs.close()


def test_fixed_record_loader_unchanged():
    import torch
    with _cluster("dram") as c:
        fs = c.client()
        d = np.random.default_rng(8).integers(0, 256, 3000 * 20, dtype=np.uint8)
        fs.write_file("/fix/part-0", d, write_type="MUST_CACHE")
        ds = FixedRecordDataset(fs, "/fix/part-0", 3000)
        with DeviceBatchLoader(ds, batch_size=8, device="cpu") as dl:
            out = list(dl)
        assert all(isinstance(t, torch.Tensor) and not isinstance(t, tuple) for t in out)
        assert [tuple(t.shape) for t in out] == [(8, 3000), (8, 3000), (4, 3000)]
        assert np.array_equal(torch.cat(out).numpy().reshape(-1), d)
        fs.close()
