"""Ragged gather on the GPU: kernel rate, loader rate, and the general path as the baseline.

Two seeded shapes (``--scale`` shrinks the record counts for a rehearsal):

* token: 1 M records of 512..8192 bytes in 2-byte multiples, batch 4096;
* image: 100 k records of 60..200 KiB, batch 256.

Per shape, from one process:

(a) kernel: ``RaggedGatherSession.raw`` over a device arena behind a scrambled 64 KiB page table,
    packed layout, align 16.  Device events bracket segments of ``--segment`` gathers that were
    queued behind a long copy, so the events see the kernels back to back and not the host's
    submission pace.  Segments alternate A/B/A/B between the two inner loops, then between
    work-item sizes; the rate is bytes delivered (record bytes) per second.
(b) loader: ``DeviceBatchLoader(device_plan="auto")`` over an HBM-tier cluster, batches per second
    and GB/s between device events on the consuming stream.
(c) the same with ``device_plan=False`` (host-planned per record and per block), alternating with (b).

The framework's batched-copy roof (one 4 GiB segment, as tools/copy_roof.py takes it) comes from
the same process.  One JSON line per measurement goes to stdout and to ``--out``.  Needs a GPU: it
fails without one.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAGE = 64 << 10
SHAPES = {
    "token": dict(records=1_000_000, lo=512, hi=8192, mult=2, batch=4096),
    "image": dict(records=100_000, lo=60 << 10, hi=200 << 10, mult=1, batch=256),
}


def lengths_of(shape, scale, seed=0):
    s = SHAPES[shape]
    n = max(s["batch"] * 4, int(s["records"] * scale))
    rng = np.random.default_rng(seed)
    return rng.integers(s["lo"] // s["mult"], s["hi"] // s["mult"] + 1, n, dtype=np.int64) * s["mult"]


def spread(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 2), "median": round(xs[len(xs) // 2], 2), "max": round(xs[-1], 2), "n": len(xs)}


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def copy_roof(torch, C, out):
    n = 4 << 30
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    src.view(torch.int64).random_()
    dst = torch.empty_like(src)
    rates = []
    for it in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        C.batched_copy([(src.data_ptr(), dst.data_ptr(), n)], 0, False)
        e1.record()
        e1.synchronize()
        if it:
            rates.append(n / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    roof = spread(rates)
    emit({"what": "copy_roof", "bytes": n, "batched_copy_kernel_GBps": roof}, out)
    return roof["median"], src, dst


def kernel_phase(torch, C, shape, lens, a, roof, blocker):
    s = SHAPES[shape]
    batch = s["batch"]
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    total = int(lens.sum())
    npages = -(-total // PAGE)
    pages = np.random.default_rng(1).permutation(npages).astype(np.int64)
    arena = torch.empty(npages * PAGE, dtype=torch.uint8, device="cuda")
    arena.view(torch.int64).random_()
    sess = C.RaggedGatherSession.raw(arena.data_ptr(), pages.tolist(), PAGE, 0, starts, lens.astype(np.uint32))
    rng = np.random.default_rng(2)
    nb = a.segment
    idx = [rng.integers(0, len(lens), batch) for _ in range(nb)]
    data_bytes = [int(lens[i].sum()) for i in idx]
    cap = max(int(((lens[i] + 15) & ~15).sum()) for i in idx)
    dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
    off = torch.empty(batch + 1, dtype=torch.int64, device="cuda")
    ln = torch.empty(batch, dtype=torch.int32, device="cuda")
    stream = int(torch.cuda.current_stream().cuda_stream)

    def segment(variant, shift):
        C.set_ragged_gather_variant(variant, shift)
        blocker()                       # the gathers queue up behind this
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t = time.perf_counter()
        for i in idx:
            sess.gather(i, dst.data_ptr(), cap, off.data_ptr(), ln.data_ptr(), "packed", 16, 0, 0, 0, 1, stream)
        host_s = time.perf_counter() - t
        e1.record()
        e1.synchronize()
        return sum(data_bytes) / (e0.elapsed_time(e1) * 1e-3) / 1e9, host_s / nb

    default_shift = C.ragged_gather_chunk_shift()
    for v in (0, 1):
        segment(v, default_shift)       # warm both code objects
    reps = -(-a.batches // nb)
    res = {0: [], 1: []}
    host = []
    for _ in range(reps):
        for v in (0, 1):                # A/B/A/B
            r, h = segment(v, default_shift)
            res[v].append(r)
            host.append(h)
    for v in (0, 1):
        sp = spread(res[v])
        emit({"what": "kernel", "shape": shape, "variant": v, "chunk_bytes": 16 << default_shift, "batch": batch,
              "batches": reps * nb, "mean_batch_bytes": int(np.mean(data_bytes)), "GBps": sp,
              "of_copy_roof": round(sp["median"] / roof, 3), "host_us_per_gather": round(1e6 * float(np.median(host)), 1)},
             a.out)
    best = 0 if spread(res[0])["median"] >= spread(res[1])["median"] else 1
    # how the record numbers reach the plan: read from the pinned buffer (default) or copied first
    up = {False: [], True: []}
    for _ in range(reps):
        for copy_first in (False, True):
            C.RaggedGatherSession.set_index_copy(copy_first)
            up[copy_first].append(segment(best, default_shift)[0])
    C.RaggedGatherSession.set_index_copy(False)
    for copy_first, xs in up.items():
        emit({"what": "kernel_index_upload", "shape": shape, "variant": best,
              "indices": "hipMemcpyAsync to a device buffer" if copy_first else "plan reads the pinned buffer",
              "GBps": spread(xs)}, a.out)
    sweep = {sh: [] for sh in (7, 8, 9, 10, 12)}
    for _ in range(max(2, reps // 2)):
        for sh in sweep:
            sweep[sh].append(segment(best, sh)[0])
    for sh, xs in sweep.items():
        emit({"what": "kernel_chunk_sweep", "shape": shape, "variant": best, "chunk_bytes": 16 << sh, "GBps": spread(xs)},
             a.out)
    # the two variants agree on one batch
    C.set_ragged_gather_variant(0, default_shift)
    sess.gather(idx[0], dst.data_ptr(), cap, off.data_ptr(), ln.data_ptr(), "packed", 16, 0, 0, 0, 1, stream)
    n0 = int(off[-1].item())
    d0 = dst[:n0].clone()
    C.set_ragged_gather_variant(1, default_shift)
    sess.gather(idx[0], dst.data_ptr(), cap, off.data_ptr(), ln.data_ptr(), "packed", 16, 0, 0, 0, 1, stream)
    same = bool(torch.equal(d0, dst[:n0]))
    C.set_ragged_gather_variant(0, default_shift)
    emit({"what": "kernel_variants_agree", "shape": shape, "equal": same}, a.out)
    if not same:
        raise SystemExit("the two inner loops disagree")
    sess.close()


def loader_phase(torch, shape, lens, a):
    from alluxio_amd.minicluster import LocalAlluxioCluster
    from alluxio_amd.models import DeviceBatchLoader, IndexedRecordDataset
    s = SHAPES[shape]
    batch = s["batch"]
    total = int(lens.sum())
    conf = {"alluxio.worker.tieredstore.level0.dirs.path": "hbm:0",
            "alluxio.worker.tieredstore.level0.dirs.quota": str(int(total * 1.1) + (512 << 20)),
            "alluxio.worker.hbm.page.size": "64KB",
            "alluxio.user.block.size.bytes.default": "64MB"}
    chunk = np.random.default_rng(3).integers(0, 256, 64 << 20, dtype=np.uint8)
    with LocalAlluxioCluster(num_workers=1, conf=conf) as c:
        fs = c.client()
        # files of about 1 GiB, cut at record boundaries
        ends = np.cumsum(lens)
        paths, offsets, first = [], [], 0
        t = time.perf_counter()
        while first < len(lens):
            base = int(ends[first - 1]) if first else 0
            last = int(np.searchsorted(ends, base + (1 << 30), side="right"))
            last = max(last, first + 1)
            off = np.concatenate([[0], ends[first:last] - base]).astype(np.int64)
            p = f"/ragged/{shape}-{len(paths):03d}"
            with fs.create_file(p, write_type="MUST_CACHE") as f:
                left = int(off[-1])
                while left:
                    n = min(left, len(chunk))
                    f.write(chunk[:n])
                    left -= n
            paths.append(p)
            offsets.append(off)
            first = last
        write_s = time.perf_counter() - t
        ds = IndexedRecordDataset(fs, paths, index=offsets, dtype="uint8", device="cuda")
        assert len(ds) == len(lens)
        emit({"what": "dataset", "shape": shape, "records": len(ds), "bytes": total, "files": len(paths),
              "write_GBps": round(total / write_s / 1e9, 2)}, a.out)
        loaders = {"auto": DeviceBatchLoader(ds, batch, shuffle=True, seed=5, device="cuda", device_plan="auto"),
                   "general": DeviceBatchLoader(ds, batch, shuffle=True, seed=5, device="cuda", device_plan=False)}
        its = {}

        def take(name, n):
            """n batches of the loader: (batches/s, GB/s) between device events, and by the host clock."""
            nbytes = got = 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            while got < n:
                if name not in its:
                    its[name] = iter(loaders[name])
                b = next(its[name], None)
                if b is None:
                    del its[name]
                    continue
                nbytes += b.data.numel()
                got += 1
            e1.record()
            e1.synchronize()
            dev_s, wall_s = e0.elapsed_time(e1) * 1e-3, time.perf_counter() - t0
            return n / dev_s, nbytes / dev_s / 1e9, n / wall_s

        # the two paths deliver the same first batch
        b0, b1 = next(iter(loaders["auto"])), next(iter(loaders["general"]))
        same = all(bool(torch.equal(x, y)) for x, y in zip(b0, b1))
        emit({"what": "loader_paths_agree", "shape": shape, "equal": same,
              "session_path": loaders["auto"]._gather is not None}, a.out)
        if not same or loaders["auto"]._gather is None:
            raise SystemExit("loader paths disagree or the session path was not taken")
        for name in loaders:
            take(name, min(20, a.segment))                    # warm
        res = {k: [] for k in loaders}
        for _ in range(-(-a.batches // a.segment)):
            for name in ("auto", "general"):                  # A/B/A/B
                res[name].append(take(name, a.segment))
        for name, xs in res.items():
            emit({"what": "loader", "shape": shape, "device_plan": "auto" if name == "auto" else False, "batch": batch,
                  "batches": len(xs) * a.segment, "batches_per_s": spread([x[0] for x in xs]),
                  "GBps": spread([x[1] for x in xs]), "host_clock_batches_per_s": spread([x[2] for x in xs])}, a.out)
        its.clear()
        for dl in loaders.values():
            dl.close()
        fs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="token,image")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the record counts (rehearsals)")
    ap.add_argument("--batches", type=int, default=200, help="timed batches per variant (at least)")
    ap.add_argument("--segment", type=int, default=50, help="batches between two device events")
    ap.add_argument("--skip-loader", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ragged_gather_bench needs a GPU: none is visible")
    from alluxio_amd.ops.native import lib
    C = lib()
    if a.out and os.path.exists(a.out):
        os.remove(a.out)
    emit({"what": "setup", "device": torch.cuda.get_device_name(0), "scale": a.scale, "segment": a.segment,
          "batches": a.batches}, a.out)
    roof, big_a, big_b = copy_roof(torch, C, a.out)

    def blocker():
        big_b.copy_(big_a)
        big_a.copy_(big_b)

    for shape in a.shapes.split(","):
        lens = lengths_of(shape, a.scale)
        kernel_phase(torch, C, shape, lens, a, roof, blocker)
    del big_a, big_b
    torch.cuda.empty_cache()
    if not a.skip_loader:
        for shape in a.shapes.split(","):
            loader_phase(torch, shape, lengths_of(shape, a.scale), a)


if __name__ == "__main__":
    main()
