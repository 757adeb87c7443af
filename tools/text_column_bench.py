"""Text columns on the GPU: the two passes (measure, emit) in both kernel variants, what a text
column adds to a batch, the gather it replaces in ``_resolve()``, and ``read_delimited_columns`` of
one text column end to end.

Two workloads, generated from a seed: ``narrow`` (CSV rows ``id,text,number`` with a text field of
about 20 bytes, every fourth one quoted with a doubled quote inside) and ``long`` (the same rows
with a quoted text field of about 2 KB in which 2 % of the bytes are quotes, all doubled).  Per
workload and batch size (``--batches``; 65536 and 4096), from one process:

(a) kernels: the file's text lies in a device arena behind an identity page table;
    ``RaggedGatherSession.raw(...).gather`` packs a batch of rows (align 16), ``field_parse_raw``
    locates the text field as a span, ``text_measure_raw`` / ``torch.cumsum`` / ``text_emit_raw``
    pack the column.  Device events bracket each call.  Rounds alternate gather / span parse /
    measure v0 / measure v1 / cumsum / emit v0 / emit v1, so the record holds the device times of
    the same batch with their spread, the text bytes per second of each pass and the ratio
    (measure + cumsum + emit of the default variant) / (gather + span parse): what the column adds
    to a batch.  Before timing, both variants and the host loops are compared byte for byte with
    each other and with ``bytes.replace`` on the host.
(b) the code ``_resolve()`` used before: ``repeat_interleave`` + ``arange`` + fancy indexing on
    the same spans, against ``extract_text(quote=None)``; both include their one readback of the
    total.  Device events around the whole call; the outputs are compared.
(c) end to end (``--e2e-mib``): a cached file of ``narrow`` rows on an HBM-tier cluster;
    ``read_delimited_columns`` of the text column (index, loader, span parse, text passes) against
    the same loader with each batch copied to the host and read with the ``csv`` module (on
    ``--host-batches`` batches; rates are file bytes per second), by the host clock around a device
    synchronise.  The columns are compared.

One JSON line per measurement goes to stdout and to ``--out``.  Needs a GPU: it fails without one.
"""
import argparse
import csv
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAGE = 64 << 10
Q = 0x22


def spread(xs, nd=3):
    xs = sorted(xs)
    return {"min": round(xs[0], nd), "median": round(xs[len(xs) // 2], nd), "max": round(xs[-1], nd), "n": len(xs)}


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


WORDS = [b"alpha", b"beta", b"gamma", b"delta", b"north", b"south", b"red", b"blue", b"seven", b"x1", b"yz"]


def _text(rng, size):
    out = b""
    while len(out) < size:
        out += WORDS[int(rng.integers(0, len(WORDS)))] + b" "
    return out[:size].rstrip(b" ") or b"a"


def narrow_rows(n, seed):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(12, 29, n)
    rows = []
    for i in range(n):
        t = _text(rng, int(sizes[i]))
        if i % 4 == 0:                                  # as csv.writer writes a field with a quote in it
            cut = len(t) // 2
            t = b'"' + t[:cut] + b'""' + t[cut:] + b'"'
        rows.append(b"%d,%s,%d\n" % (i, t, int(sizes[i]) * 7919))
    return rows


def long_rows(n, seed, pool=256):
    """n rows drawn from a pool of distinct rows; the text field: about 2 KB, quoted, 2 % quote bytes."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(pool):
        t = bytearray(_text(rng, int(rng.integers(1800, 2300))))
        for k in rng.choice(len(t) // 3 - 1, len(t) // 100, replace=False):
            t[3 * k:3 * k + 2] = b'""'                    # pairs that never touch: the field stays well-formed
        rows.append(b'%d,"%s",%d\n' % (i, bytes(t), i * 31))
    return [rows[i] for i in rng.integers(0, pool, n)]


def kernel_phase(torch, C, name, rows, batch, a):
    from alluxio_amd.models import extract_text, split_row
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
    st = torch.empty(batch, dtype=torch.int64, device="cuda")
    le = torch.empty(batch, dtype=torch.int32, device="cuda")
    status = torch.empty(batch, dtype=torch.uint8, device="cuda")
    out_len = {v: torch.empty(batch, dtype=torch.int32, device="cuda") for v in (0, 1)}
    offsets = torch.zeros(batch + 1, dtype=torch.int64, device="cuda")

    def gather():
        g.gather(idx, data.data_ptr(), data.numel(), off.data_ptr(), ln.data_ptr(), "packed", 16, 0, 0, 0, 1, stream)

    def span():
        C.field_parse_raw(data.data_ptr(), data.numel(), off.data_ptr(), ln.data_ptr(), False, batch, 0,
                          [(1, 0, st.data_ptr(), le.data_ptr(), status.data_ptr())], 44, Q, 10, stream)

    def measure(v):
        C.set_text_column_variant(v)
        C.text_measure_raw(data.data_ptr(), data.numel(), st.data_ptr(), le.data_ptr(), status.data_ptr(), batch, 0, Q,
                           out_len[v].data_ptr(), stream)

    def scan():
        torch.cumsum(out_len[1], 0, dtype=torch.int64, out=offsets[1:])

    default = C.text_column_variant()
    try:
        gather()
        span()
        measure(0)
        measure(1)
        scan()
        total = int(offsets[-1])
        packed = {v: torch.empty(total, dtype=torch.uint8, device="cuda") for v in (0, 1)}

        def emit_text(v):
            C.set_text_column_variant(v)
            C.text_emit_raw(data.data_ptr(), data.numel(), st.data_ptr(), le.data_ptr(), status.data_ptr(), batch, 0, Q,
                            offsets.data_ptr(), packed[v].data_ptr(), total, stream)

        emit_text(0)
        emit_text(1)
        torch.cuda.synchronize()
        # both variants, the host loops and bytes.replace agree, and every value is valid
        if not (status == 0).all():
            raise SystemExit(f"{name}: span statuses {torch.unique(status).tolist()}")
        known = {}                                      # the long rows come from a pool: each is split once
        for r in rows:
            if r not in known:
                known[r] = split_row(r, quote='"')[1].replace(b'""', b'"')
        want = b"".join(known[rows[i]] for i in idx)
        h_data, h_st, h_le = data.cpu().numpy(), st.cpu().numpy(), le.cpu().numpy()
        h_len = np.empty(batch, np.int32)
        C.text_measure_raw(h_data.ctypes.data, h_data.size, h_st.ctypes.data, h_le.ctypes.data, 0, batch, -1, Q,
                           h_len.ctypes.data, 0)
        h_off = np.concatenate([[0], np.cumsum(h_len, dtype=np.int64)])
        h_out = np.empty(int(h_off[-1]), np.uint8)
        t0 = time.perf_counter()
        C.text_emit_raw(h_data.ctypes.data, h_data.size, h_st.ctypes.data, h_le.ctypes.data, 0, batch, -1, Q,
                        h_off.ctypes.data, h_out.ctypes.data, h_out.size, 0)
        host_emit_ms = (time.perf_counter() - t0) * 1e3
        if h_out.tobytes() != want:
            raise SystemExit(f"{name}: the host loop differs from bytes.replace")
        for v in (0, 1):
            if not (np.array_equal(out_len[v].cpu().numpy(), h_len) and packed[v].cpu().numpy().tobytes() == want):
                raise SystemExit(f"{name}: variant {v} differs from the host loop")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def timed(fn):
            ev[0].record()
            fn()
            ev[1].record()
            ev[1].synchronize()
            return ev[0].elapsed_time(ev[1])

        steps = [("gather", gather), ("span", span), ("measure0", lambda: measure(0)), ("measure1", lambda: measure(1)),
                 ("cumsum", scan), ("emit0", lambda: emit_text(0)), ("emit1", lambda: emit_text(1))]
        times = {k: [] for k, _ in steps}
        for it in range(a.warmup + a.rounds):
            for k, fn in steps:                         # the candidates alternate inside a round
                ms = timed(fn)
                if it >= a.warmup:
                    times[k].append(ms)

        # (b) the gather that _resolve() used, on the same spans, against extract_text without a quote
        flat = data

        def old():
            l64 = le.to(torch.int64)
            ends = torch.cumsum(l64, 0)
            pos = torch.repeat_interleave(st - (ends - l64), l64) + torch.arange(int(ends[-1]), device=flat.device)
            return flat[pos]

        def new():
            return extract_text(flat, st, le).data

        C.set_text_column_variant(default)
        if not torch.equal(old(), new()):
            raise SystemExit(f"{name}: extract_text differs from the index gather")
        both = {"index_gather": [], "extract_text": []}
        for it in range(a.warmup + a.rounds):
            for k, fn in (("index_gather", old), ("extract_text", new)):
                ms = timed(fn)
                if it >= a.warmup:
                    both[k].append(ms)
    finally:
        C.set_text_column_variant(default)
        g.close()
    med = {k: spread(v)["median"] for k, v in times.items()}
    in_bytes = int(h_le.sum())
    adds = med[f"measure{default}"] + med["cumsum"] + med[f"emit{default}"]
    emit({"what": "kernels", "workload": name, "batch": batch, "row_bytes": int(lens.sum()), "text_bytes": in_bytes,
          "out_bytes": total, "mean_text": round(in_bytes / batch, 1),
          **{k + "_ms": spread(v) for k, v in times.items()},
          "measure_v0_GBps": round(in_bytes / med["measure0"] / 1e6, 2),
          "measure_v1_GBps": round(in_bytes / med["measure1"] / 1e6, 2),
          "emit_v0_GBps": round(in_bytes / med["emit0"] / 1e6, 2), "emit_v1_GBps": round(in_bytes / med["emit1"] / 1e6, 2),
          "measure_v0_over_v1": round(med["measure0"] / med["measure1"], 2),
          "emit_v0_over_v1": round(med["emit0"] / med["emit1"], 2), "default_variant": default,
          "column_ms": round(adds, 3), "gather_plus_span_ms": round(med["gather"] + med["span"], 3),
          "column_over_gather_plus_span": round(adds / (med["gather"] + med["span"]), 2),
          "host_emit_ms": round(host_emit_ms, 2), "equal": True}, a.out)
    mo, mn = spread(both["index_gather"])["median"], spread(both["extract_text"])["median"]
    emit({"what": "resolve_gather", "workload": name, "batch": batch, "text_bytes": in_bytes,
          "index_gather_ms": spread(both["index_gather"]), "extract_text_ms": spread(both["extract_text"]),
          "speedup": round(mo / mn, 2), "equal": True}, a.out)


def e2e_phase(torch, size, a):
    from alluxio_amd.minicluster import LocalAlluxioCluster
    from alluxio_amd.models import DeviceBatchLoader, IndexedRecordDataset, read_delimited_columns
    conf = {"alluxio.worker.tieredstore.level0.dirs.path": "hbm:0",
            "alluxio.worker.tieredstore.level0.dirs.quota": str(size + (512 << 20)),
            "alluxio.worker.hbm.page.size": "64KB",
            "alluxio.user.block.size.bytes.default": "64MB"}
    chunk = b"".join(narrow_rows(65536, 11))
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
            got = read_delimited_columns(fs, "/text/e2e.csv", [(1, "text")], quote='"', batch_size=65536, device="cuda")
            torch.cuda.synchronize()
            if it:
                dev_ms.append((time.perf_counter() - t) * 1e3)
        col = got[0]
        cuts = col.offsets.cpu().numpy()
        packed = col.data.cpu().numpy().tobytes()
        ds = IndexedRecordDataset.from_delimited(fs, "/text/e2e.csv", quote='"', device="cuda")
        host_s, host_bytes, nb, same = 0.0, 0, 0, True
        with DeviceBatchLoader(ds, batch_size=65536, device="cuda", align=1) as dl:
            for batch in dl:
                t = time.perf_counter()
                data, off, ln = (x.cpu().numpy() for x in batch)
                buf = data.tobytes().decode()
                names = [r[1] for r in csv.reader(io.StringIO(buf, newline=""))]
                host_s += time.perf_counter() - t
                lo = nb * 65536
                mine = [packed[cuts[lo + j]:cuts[lo + j + 1]].decode() for j in range(len(names))]
                same = same and mine == names
                host_bytes += int(ln.sum())
                nb += 1
                if nb >= a.host_batches:
                    break
        dev_rate = written / spread(dev_ms)["median"] / 1e6
        host_rate = host_bytes / host_s / 1e9
        emit({"what": "end_to_end", "file_mib": written >> 20, "rows": got.rows, "text_bytes": len(packed),
              "read_delimited_columns_ms": spread(dev_ms, 1), "device_GBps": round(dev_rate, 2),
              "host_csv_batches": nb, "host_csv_GBps": round(host_rate, 4), "speedup": round(dev_rate / host_rate, 1),
              "equal_on_host_batches": same}, a.out)
        fs.close()
        if not same:
            raise SystemExit("the device column and the csv module's column differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="65536,4096")
    ap.add_argument("--workloads", default="narrow,long")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e-mib", type=int, default=256, help="file of the end-to-end phase (0: skip)")
    ap.add_argument("--e2e-rounds", type=int, default=3)
    ap.add_argument("--host-batches", type=int, default=2, help="batches the csv module reads")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("text_column_bench needs a GPU: none is visible")
    from alluxio_amd.ops.native import lib
    C = lib()
    if a.out and os.path.exists(a.out):
        os.remove(a.out)
    emit({"what": "setup", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup,
          "default_variant": C.text_column_variant()}, a.out)
    batches = [int(b) for b in a.batches.split(",")]
    for name in a.workloads.split(","):
        rows = (narrow_rows if name == "narrow" else long_rows)(max(batches), 5)
        for b in batches:
            kernel_phase(torch, C, name, rows, b, a)
    if a.e2e_mib:
        e2e_phase(torch, a.e2e_mib << 20, a)


if __name__ == "__main__":
    main()
