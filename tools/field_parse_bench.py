"""Field parse on the GPU: the parse kernel against the gather that produced its batch, against the
host loop, and ``read_delimited_columns`` end to end.

Two workloads, generated from a seed: ``narrow`` (CSV rows of about 100 bytes, 8 numeric fields, all
requested) and ``wide`` (rows of about 4 KiB, 200 fields, 4 requested).  Per workload and batch size
(``--batches``; 65536 for both and 4096 as a third point), from one process:

(a) kernels: the file's text lies in a device arena behind an identity page table;
    ``RaggedGatherSession.raw(...).gather`` packs a batch of rows (align 16) and ``field_parse_raw``
    parses that batch.  Device events bracket each call.  Rounds alternate gather / parse variant 0 /
    parse variant 1 (A/B/C/A/B/C), so the record holds the three device times of the same batch with
    their spread, the row bytes per second of the parse and the ratio parse / gather.  The gather's
    time includes its index copy and its plan launch.  Before timing, both variants and the host
    loop are compared column by column (bit patterns) and every status must be 0.
(b) host loop: ``field_parse_raw(device=-1)`` on the same bytes in host memory, by the host clock.
(c) end to end (``--e2e-mib``): a cached file of ``narrow`` rows on an HBM-tier cluster;
    ``read_delimited_columns`` (index, loader, parse) against the same loader with each batch copied
    to the host and parsed there with ``bytes.split`` + ``int`` / ``float`` (on ``--host-batches``
    batches; rates are file bytes per second), by the host clock around a device synchronise.

One JSON line per measurement goes to stdout and to ``--out``.  Needs a GPU: it fails without one.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAGE = 64 << 10
I64, I32, F64, F32 = 1, 2, 3, 4
NP = {I64: np.int64, I32: np.int32, F64: np.float64, F32: np.float32}


def spread(xs, nd=3):
    xs = sorted(xs)
    return {"min": round(xs[0], nd), "median": round(xs[len(xs) // 2], nd), "max": round(xs[-1], nd), "n": len(xs)}


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def narrow_rows(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 10 ** 9, (n, 3))
    x = rng.standard_normal((n, 5)) * 1000
    return [b"%d,%.6f,%.6f,%.6f,%d,%d,%.5e,%.5e\n" % (a[i, 0], x[i, 0], x[i, 1], x[i, 2], a[i, 1] - 5 * 10 ** 8, a[i, 2] % 10 ** 7,
                                                    x[i, 3], x[i, 4]) for i in range(n)]


NARROW_COLS = [(0, I64), (1, F64), (2, F64), (3, F32), (4, I64), (5, I32), (6, F64), (7, F32)]
WIDE_COLS = [(3, I64), (60, F64), (120, F32), (199, I32)]


def wide_rows(n, seed, pool=256):
    """n rows of 200 fields drawn from a pool of distinct rows: ints and decimals of about 19 bytes."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(pool):
        v = rng.integers(-10 ** 17, 10 ** 17, 100)
        x = rng.standard_normal(100) * 1e3
        cells = [b"%d" % v[j // 2] if j % 4 == 3 else (b"%.8f" % x[j // 2] if j % 2 == 0 else b"%d" % (v[j // 2] % 10 ** 9))
                 for j in range(200)]
        cells[199] = b"%d" % (v[99] % 2 ** 31)
        pad = [c + b" " * max(0, 19 - len(c)) for c in cells]       # blanks are trimmed by the rule
        rows.append(b",".join(pad) + b"\n")
    return [rows[i] for i in rng.integers(0, pool, n)]


def columns(torch, cols, n, device):
    outs, raw = [], []
    for k, t in cols:
        if device == "cuda":
            v = torch.empty(n, dtype=getattr(torch, np.dtype(NP[t]).name), device="cuda")
            st = torch.empty(n, dtype=torch.uint8, device="cuda")
            raw.append((k, t, v.data_ptr(), 0, st.data_ptr()))
        else:
            v, st = np.empty(n, NP[t]), np.empty(n, np.uint8)
            raw.append((k, t, v.ctypes.data, 0, st.ctypes.data))
        outs.append((v, st))
    return outs, raw


def kernel_phase(torch, C, name, rows, cols, batch, a):
    rows = rows[:batch]
    lens = np.array([len(r) for r in rows], dtype=np.uint32)
    starts = np.concatenate([[0], np.cumsum(lens, dtype=np.uint64)[:-1]]).astype(np.uint64)
    text = np.frombuffer(b"".join(rows), dtype=np.uint8)
    npages = (text.size + PAGE - 1) // PAGE
    arena = torch.zeros(npages * PAGE, dtype=torch.uint8, device="cuda")
    arena[:text.size] = torch.from_numpy(text.copy()).cuda()
    g = C.RaggedGatherSession.raw(arena.data_ptr(), list(range(npages)), PAGE, 0, starts, lens)
    idx = np.random.default_rng(3).permutation(batch).astype(np.int64)      # a shuffled batch
    adv = (lens[idx].astype(np.int64) + 15) & ~15
    data = torch.empty(int(adv.sum()), dtype=torch.uint8, device="cuda")
    off = torch.empty(batch + 1, dtype=torch.int64, device="cuda")
    ln = torch.empty(batch, dtype=torch.int32, device="cuda")
    stream = int(torch.cuda.current_stream().cuda_stream)
    row_bytes = int(lens.sum())

    def gather():
        g.gather(idx, data.data_ptr(), data.numel(), off.data_ptr(), ln.data_ptr(), "packed", 16, 0, 0, 0, 1, stream)

    outs = {v: columns(torch, cols, batch, "cuda") for v in (0, 1)}

    def parse(v):
        C.set_field_parse_variant(v)
        C.field_parse_raw(data.data_ptr(), data.numel(), off.data_ptr(), ln.data_ptr(), False, batch, 0, outs[v][1],
                          44, -1, 10, stream)

    default = C.field_parse_variant()
    try:
        gather()
        parse(0)
        parse(1)
        torch.cuda.synchronize()
        # the same columns from both variants and from the host loop, and nothing malformed or deferred
        h_data, h_off, h_ln = data.cpu().numpy(), off.cpu().numpy(), ln.cpu().numpy()
        h_outs, h_raw = columns(torch, cols, batch, "cpu")
        host_ms = []
        for _ in range(a.host_rounds):
            t = time.perf_counter()
            C.field_parse_raw(h_data.ctypes.data, h_data.size, h_off.ctypes.data, h_ln.ctypes.data, False, batch, -1, h_raw,
                              44, -1, 10, 0)
            host_ms.append((time.perf_counter() - t) * 1e3)
        for j, (k, t) in enumerate(cols):
            iv = np.int64 if NP[t]().itemsize == 8 else np.int32
            want, wst = h_outs[j][0].view(iv), h_outs[j][1]
            if not (wst == 0).all():
                raise SystemExit(f"{name}: column {k} has statuses {np.unique(wst).tolist()}")
            for v in (0, 1):
                if not (np.array_equal(outs[v][0][j][0].cpu().numpy().view(iv), want)
                        and np.array_equal(outs[v][0][j][1].cpu().numpy(), wst)):
                    raise SystemExit(f"{name}: variant {v} differs from the host loop in column {k}")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def timed(fn):
            ev[0].record()
            fn()
            ev[1].record()
            ev[1].synchronize()
            return ev[0].elapsed_time(ev[1])

        times = {"gather": [], 0: [], 1: []}
        for it in range(a.warmup + a.rounds):
            for what in ("gather", 0, 1):               # A/B/C/A/B/C
                ms = timed(gather if what == "gather" else (lambda: parse(what)))
                if it >= a.warmup:
                    times[what].append(ms)
    finally:
        C.set_field_parse_variant(default)
        g.close()
    med = {k: spread(v)["median"] for k, v in times.items()}
    emit({"what": "kernels", "workload": name, "batch": batch, "row_bytes": row_bytes, "mean_row": round(row_bytes / batch, 1),
          "columns": len(cols), "gather_ms": spread(times["gather"]), "parse_v0_ms": spread(times[0]),
          "parse_v1_ms": spread(times[1]),
          "parse_v0_GBps": round(row_bytes / med[0] / 1e6, 2), "parse_v1_GBps": round(row_bytes / med[1] / 1e6, 2),
          "gather_GBps": round(row_bytes / med["gather"] / 1e6, 2),
          "v0_over_gather": round(med[0] / med["gather"], 2), "v1_over_gather": round(med[1] / med["gather"], 2),
          "v0_over_v1": round(med[0] / med[1], 2), "host_loop_ms": spread(host_ms),
          "host_loop_GBps": round(row_bytes / spread(host_ms)["median"] / 1e6, 3), "equal": True}, a.out)


def python_parse(data, off, ln):
    """What a training loop does without the kernel: the batch on the host, split and converted."""
    buf = data.tobytes()
    cols = [[] for _ in range(8)]
    for o, n in zip(off.tolist(), ln.tolist()):
        f = buf[o:o + n].rstrip(b"\n").split(b",")
        cols[0].append(int(f[0]))
        cols[1].append(float(f[1]))
        cols[2].append(float(f[2]))
        cols[3].append(float(f[3]))
        cols[4].append(int(f[4]))
        cols[5].append(int(f[5]))
        cols[6].append(float(f[6]))
        cols[7].append(float(f[7]))
    return [np.array(c, dtype=NP[t]) for c, (_, t) in zip(cols, NARROW_COLS)]


def e2e_phase(torch, size, a):
    from alluxio_amd.minicluster import LocalAlluxioCluster
    from alluxio_amd.models import DeviceBatchLoader, IndexedRecordDataset, read_delimited_columns
    conf = {"alluxio.worker.tieredstore.level0.dirs.path": "hbm:0",
            "alluxio.worker.tieredstore.level0.dirs.quota": str(size + (512 << 20)),
            "alluxio.worker.hbm.page.size": "64KB",
            "alluxio.user.block.size.bytes.default": "64MB"}
    chunk = b"".join(narrow_rows(65536, 11))
    names = {1: "int64", 2: "int32", 3: "float64", 4: "float32"}
    cols = [(k, names[t]) for k, t in NARROW_COLS]
    with LocalAlluxioCluster(num_workers=1, conf=conf) as c:
        fs = c.client()
        written = 0
        with fs.create_file("/text/e2e.csv", write_type="MUST_CACHE") as f:
            while written + len(chunk) <= size:
                f.write(chunk)
                written += len(chunk)
        dev_ms, got = [], None
        for it in range(a.e2e_rounds + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            got = read_delimited_columns(fs, "/text/e2e.csv", cols, batch_size=65536, device="cuda")
            torch.cuda.synchronize()
            if it:
                dev_ms.append((time.perf_counter() - t) * 1e3)
        # the host path on the first batches of the same loader
        ds = IndexedRecordDataset.from_delimited(fs, "/text/e2e.csv", device="cuda")
        host_s, host_bytes, nb, same = 0.0, 0, 0, True
        with DeviceBatchLoader(ds, batch_size=65536, device="cuda", align=1) as dl:
            for batch in dl:
                t = time.perf_counter()
                data, off, ln = (x.cpu().numpy() for x in batch)
                parsed = python_parse(data, off, ln)
                host_s += time.perf_counter() - t
                lo = nb * 65536
                for j, p in enumerate(parsed):
                    iv = np.int64 if p.itemsize == 8 else np.int32
                    same = same and bool(np.array_equal(got[j].values[lo:lo + len(p)].cpu().numpy().view(iv), p.view(iv)))
                host_bytes += int(ln.sum())
                nb += 1
                if nb >= a.host_batches:
                    break
        statuses = sorted({int(s) for col in got for s in torch.unique(col.status).tolist()})
        dev_rate = written / spread(dev_ms)["median"] / 1e6
        host_rate = host_bytes / host_s / 1e9
        emit({"what": "end_to_end", "file_mib": written >> 20, "rows": got.rows, "columns": len(cols),
              "read_delimited_columns_ms": spread(dev_ms, 1), "device_GBps": round(dev_rate, 2),
              "host_python_batches": nb, "host_python_GBps": round(host_rate, 4), "speedup": round(dev_rate / host_rate, 1),
              "statuses": statuses, "equal_on_host_batches": same}, a.out)
        fs.close()
        if not same or statuses != [0]:
            raise SystemExit("the device columns and the host columns differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="65536,4096")
    ap.add_argument("--workloads", default="narrow,wide")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--e2e-mib", type=int, default=1024, help="file of the end-to-end phase (0: skip)")
    ap.add_argument("--e2e-rounds", type=int, default=3)
    ap.add_argument("--host-batches", type=int, default=4, help="batches the host path parses")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("field_parse_bench needs a GPU: none is visible")
    from alluxio_amd.ops.native import lib
    C = lib()
    if a.out and os.path.exists(a.out):
        os.remove(a.out)
    emit({"what": "setup", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup,
          "default_variant": C.field_parse_variant()}, a.out)
    batches = [int(b) for b in a.batches.split(",")]
    for name in a.workloads.split(","):
        rows = (narrow_rows if name == "narrow" else wide_rows)(max(batches), 5)
        cols = NARROW_COLS if name == "narrow" else WIDE_COLS
        for b in batches:
            kernel_phase(torch, C, name, rows, cols, b, a)
    if a.e2e_mib:
        e2e_phase(torch, a.e2e_mib << 20, a)


if __name__ == "__main__":
    main()
