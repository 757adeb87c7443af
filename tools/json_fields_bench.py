"""JSON Lines columns on the GPU: the locate pass and the two unescape passes in both kernel
variants, against the gather that produced the batch and against ``parse_fields`` on a CSV batch of
the same values, and ``read_json_columns`` end to end against ``json.loads`` per row on the host.

Two batches, generated from a seed: ``scalars`` (65,536 rows of about 120 bytes with 6 scalar keys,
all requested: two ints, two floats, a bool and a short label located as a string) and ``text``
(4,096 rows of about 4 KB whose ``"text"`` value is about 3.8 KB with a ``\\n`` every 60 bytes or
so; ``id`` and ``text`` requested).  Per batch, from one process:

(a) kernels: the file's text lies in a device arena behind an identity page table;
    ``RaggedGatherSession.raw(...).gather`` packs a shuffled batch of rows (align 16);
    ``json_fields_raw`` locates and types the keys; for ``text``, ``json_text_measure_raw`` /
    ``torch.cumsum`` / ``json_text_emit_raw`` pack the column.  The same values written as CSV rows
    go through the same gather and ``field_parse_raw`` (and ``text_measure_raw`` / ``text_emit_raw``
    for the text field) in their default variants.  Device events bracket each call and the
    candidates alternate inside a round.  Before timing, both variants and the host loops are
    compared byte for byte with each other, and the values with ``json.loads``.
(b) end to end (``--e2e-mib``): a cached file of each workload on an HBM-tier cluster;
    ``read_json_columns`` (index, loader, locate, unescape, concatenation) against the same loader
    with each batch copied to the host and read with ``json.loads`` per row (on ``--host-batches``
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
WORDS = ["alpha", "beta", "gamma", "delta", "north", "south", "red", "blue", "seven", "x1", "yz", "café"]
SCALAR_COLS = [("id", 1), ("count", 2), ("score", 3), ("ratio", 4), ("ok", 5), ("label", 6)]      # raw type codes
TEXT_COLS = [("id", 1), ("text", 6)]


def spread(xs, nd=3):
    xs = sorted(xs)
    return {"min": round(xs[0], nd), "median": round(xs[len(xs) // 2], nd), "max": round(xs[-1], nd), "n": len(xs)}


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def scalar_objects(n, seed):
    rng = np.random.default_rng(seed)
    a, b, c = rng.integers(-10 ** 9, 10 ** 9, n), rng.integers(0, 10 ** 6, n), rng.integers(0, 2, n)
    return [{"id": i, "count": int(a[i]), "score": int(b[i]) / 64.0, "ratio": round(int(b[i]) * 1e-3, 3), "ok": bool(c[i]),
             "label": WORDS[int(b[i]) % 11] + "-" + WORDS[int(a[i]) % 11], "pad": "x" * int(b[i] % 17)} for i in range(n)]


def text_objects(n, seed, pool=256):
    rng = np.random.default_rng(seed)
    texts = []
    for _ in range(pool):
        lines, size = [], 0
        while size < 3700:
            ln = " ".join(WORDS[int(k)] for k in rng.integers(0, len(WORDS), int(rng.integers(8, 13))))
            lines.append(ln)
            size += len(ln) + 2
        texts.append("\n".join(lines))
    pick = rng.integers(0, pool, n)
    return [{"id": i, "meta": {"src": "pool", "n": int(pick[i])}, "text": texts[int(pick[i])], "lang": "en"} for i in range(n)]


def as_jsonl(objs):
    return [(json.dumps(o, ensure_ascii=False, separators=(",", ":")) + "\n").encode() for o in objs]


def as_csv(objs, name):
    if name == "scalars":
        return [b"%d,%d,%r,%r,%s,%s,%s\n" % (o["id"], o["count"], o["score"], o["ratio"], str(o["ok"]).lower().encode(),
                                            o["label"].encode(), o["pad"].encode()) for o in objs]
    return [b'%d,"%s",en\n' % (o["id"], o["text"].replace('"', '""').encode()) for o in objs]


class Batch:
    """The rows in a device arena, and one shuffled packed batch of them."""

    def __init__(self, torch, C, rows, batch):
        self.torch, self.C, self.n = torch, C, batch
        rows = rows[:batch]
        lens = np.array([len(r) for r in rows], dtype=np.uint32)
        starts = np.concatenate([[0], np.cumsum(lens, dtype=np.uint64)[:-1]]).astype(np.uint64)
        text = np.frombuffer(b"".join(rows), dtype=np.uint8)
        npages = (text.size + PAGE - 1) // PAGE
        self.arena = torch.zeros(npages * PAGE, dtype=torch.uint8, device="cuda")
        self.arena[:text.size] = torch.from_numpy(text.copy()).cuda()
        self.g = C.RaggedGatherSession.raw(self.arena.data_ptr(), list(range(npages)), PAGE, 0, starts, lens)
        self.idx = np.random.default_rng(3).permutation(batch).astype(np.int64)
        adv = (lens[self.idx].astype(np.int64) + 15) & ~15
        self.data = torch.empty(int(adv.sum()), dtype=torch.uint8, device="cuda")
        self.off = torch.empty(batch + 1, dtype=torch.int64, device="cuda")
        self.ln = torch.empty(batch, dtype=torch.int32, device="cuda")
        self.row_bytes = int(lens.sum())
        self.stream = int(torch.cuda.current_stream().cuda_stream)

    def gather(self):
        self.g.gather(self.idx, self.data.data_ptr(), self.data.numel(), self.off.data_ptr(), self.ln.data_ptr(), "packed", 16,
                      0, 0, 0, 1, self.stream)


def _outputs(torch, cols, n, device):
    dt = {1: torch.int64, 2: torch.int32, 3: torch.float64, 4: torch.float32, 5: torch.uint8, 6: torch.int64, 0: torch.int64}
    return [(torch.zeros(n, dtype=dt[t], device=device), torch.zeros(n, dtype=torch.int32, device=device),
             torch.zeros(n, dtype=torch.uint8, device=device)) for _, t in cols]


def kernel_phase(torch, C, name, objs, batch, a):
    cols = SCALAR_COLS if name == "scalars" else TEXT_COLS
    jb = Batch(torch, C, as_jsonl(objs), batch)
    cb = Batch(torch, C, as_csv(objs, name), batch)
    names = b"".join(k.encode() for k, _ in cols)
    d_names = torch.from_numpy(np.frombuffer(names, dtype=np.uint8).copy()).cuda()
    outs = {v: _outputs(torch, cols, batch, "cuda") for v in (0, 1)}

    def spec(outs_v, ptr):
        at, sp = 0, []
        for (k, t), (val, ln, st) in zip(cols, outs_v):
            sp.append((at, len(k.encode()), t, ptr(val), ptr(ln), ptr(st)))
            at += len(k.encode())
        return sp

    def locate(v):
        C.set_json_fields_variant(v)
        C.json_fields_raw(jb.data.data_ptr(), jb.data.numel(), jb.off.data_ptr(), jb.ln.data_ptr(), False, batch, 0,
                          d_names.data_ptr(), len(names), spec(outs[v], lambda x: x.data_ptr()), 10, jb.stream)

    # the CSV batch: the same values through field_parse_raw in its default variant
    csv_types = [1, 2, 3, 4, 0, 0] if name == "scalars" else [1, 0]
    c_outs = _outputs(torch, [(None, t) for t in csv_types], batch, "cuda")

    def csv_parse():
        C.field_parse_raw(cb.data.data_ptr(), cb.data.numel(), cb.off.data_ptr(), cb.ln.data_ptr(), False, batch, 0,
                          [(j, t, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr()) for j, (t, o) in
                           enumerate(zip(csv_types, c_outs))], 44, 0x22, 10, cb.stream)

    d_fields, d_text = C.json_fields_variant(), C.json_text_variant()
    try:
        jb.gather()
        cb.gather()
        locate(0)
        locate(1)
        csv_parse()
        torch.cuda.synchronize()
        # the host loop on the same batch
        h_data, h_off, h_ln = jb.data.cpu().numpy(), jb.off.cpu().numpy(), jb.ln.cpu().numpy()
        h_names = np.frombuffer(names, dtype=np.uint8).copy()
        h_outs = _outputs(torch, cols, batch, "cpu")
        host_ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            C.json_fields_raw(h_data.ctypes.data, h_data.size, h_off.ctypes.data, h_ln.ctypes.data, False, batch, -1,
                              h_names.ctypes.data, len(names), spec(h_outs, lambda x: x.data_ptr()), 10, 0)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        for v in (0, 1):
            for (k, t), dev, host in zip(cols, outs[v], h_outs):
                for x, y in zip(dev, host):
                    if not torch.equal(x.cpu().view(torch.uint8), y.view(torch.uint8)):
                        raise SystemExit(f"{name}: variant {v} differs from the host loop in column {k}")
        picked = [objs[i] for i in jb.idx]
        for (k, t), (val, ln, st) in zip(cols, h_outs):
            if t == 6:
                continue
            want = [o[k] for o in picked] if t != 4 else np.array([o[k] for o in picked], dtype=np.float32).tolist()
            if not (st == 0).all() or val.tolist() != want:
                raise SystemExit(f"{name}: column {k} differs from json.loads")
        steps = [("gather", jb.gather), ("locate0", lambda: locate(0)), ("locate1", lambda: locate(1)),
                 ("csv_gather", cb.gather), ("csv_parse", csv_parse)]
        text_bytes = 0
        if name == "text":
            ti = [k for k, _ in cols].index("text")
            st_, le_, status = outs[1][ti]
            out_len = {v: torch.empty(batch, dtype=torch.int32, device="cuda") for v in (0, 1)}
            out_st = {v: torch.empty(batch, dtype=torch.uint8, device="cuda") for v in (0, 1)}
            offsets = torch.zeros(batch + 1, dtype=torch.int64, device="cuda")

            def measure(v):
                C.set_json_text_variant(v)
                C.json_text_measure_raw(jb.data.data_ptr(), jb.data.numel(), st_.data_ptr(), le_.data_ptr(), status.data_ptr(),
                                        batch, 0, out_len[v].data_ptr(), out_st[v].data_ptr(), jb.stream)

            def scan():
                torch.cumsum(out_len[1], 0, dtype=torch.int64, out=offsets[1:])

            measure(0)
            measure(1)
            scan()
            total = int(offsets[-1])
            packed = {v: torch.empty(total, dtype=torch.uint8, device="cuda") for v in (0, 1)}

            def emit_text(v):
                C.set_json_text_variant(v)
                C.json_text_emit_raw(jb.data.data_ptr(), jb.data.numel(), st_.data_ptr(), le_.data_ptr(), out_st[v].data_ptr(),
                                     batch, 0, offsets.data_ptr(), packed[v].data_ptr(), total, jb.stream)

            emit_text(0)
            emit_text(1)
            torch.cuda.synchronize()
            want = b"".join(o["text"].encode() for o in picked)
            for v in (0, 1):
                if not (out_st[v] == 0).all() or packed[v].cpu().numpy().tobytes() != want:
                    raise SystemExit(f"{name}: unescape variant {v} differs from json.loads")
            text_bytes = int(le_.sum())
            # the CSV text field: span -> text_measure_raw / text_emit_raw in their default variant
            c_len = torch.empty(batch, dtype=torch.int32, device="cuda")
            c_offsets = torch.zeros(batch + 1, dtype=torch.int64, device="cuda")
            c_packed = torch.empty(total + 16, dtype=torch.uint8, device="cuda")

            def csv_text():
                s, l, u = c_outs[1]
                C.text_measure_raw(cb.data.data_ptr(), cb.data.numel(), s.data_ptr(), l.data_ptr(), u.data_ptr(), batch, 0, 0x22,
                                   c_len.data_ptr(), cb.stream)
                torch.cumsum(c_len, 0, dtype=torch.int64, out=c_offsets[1:])
                C.text_emit_raw(cb.data.data_ptr(), cb.data.numel(), s.data_ptr(), l.data_ptr(), u.data_ptr(), batch, 0, 0x22,
                                c_offsets.data_ptr(), c_packed.data_ptr(), c_packed.numel(), cb.stream)

            steps += [("measure0", lambda: measure(0)), ("measure1", lambda: measure(1)), ("cumsum", scan),
                      ("emit0", lambda: emit_text(0)), ("emit1", lambda: emit_text(1)), ("csv_text", csv_text)]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def timed(fn):
            ev[0].record()
            fn()
            ev[1].record()
            ev[1].synchronize()
            return ev[0].elapsed_time(ev[1])

        times = {k: [] for k, _ in steps}
        for it in range(a.warmup + a.rounds):
            for k, fn in steps:                         # the candidates alternate inside a round
                ms = timed(fn)
                if it >= a.warmup:
                    times[k].append(ms)
    finally:
        C.set_json_fields_variant(d_fields)
        C.set_json_text_variant(d_text)
        jb.g.close()
        cb.g.close()
    med = {k: spread(v)["median"] for k, v in times.items()}
    rec = {"what": "kernels", "workload": name, "batch": batch, "row_bytes": jb.row_bytes, "csv_row_bytes": cb.row_bytes,
           "columns": len(cols), **{k + "_ms": spread(v) for k, v in times.items()},
           "locate_v0_over_v1": round(med["locate0"] / med["locate1"], 2),
           "locate_v0_over_gather": round(med["locate0"] / med["gather"], 2),
           "locate_v1_over_gather": round(med["locate1"] / med["gather"], 2),
           "locate_v1_GBps": round(jb.row_bytes / med["locate1"] / 1e6, 1),
           "locate_v0_over_csv_parse": round(med["locate0"] / med["csv_parse"], 2),
           "locate_v1_over_csv_parse": round(med["locate1"] / med["csv_parse"], 2),
           "host_loop_ms": spread(host_ms, 2), "default_fields_variant": d_fields, "default_text_variant": d_text, "equal": True}
    if name == "text":
        rec.update({"text_bytes": text_bytes, "measure_v0_over_v1": round(med["measure0"] / med["measure1"], 2),
                    "emit_v0_over_v1": round(med["emit0"] / med["emit1"], 2),
                    "measure_v1_GBps": round(text_bytes / med["measure1"] / 1e6, 1),
                    "emit_v1_GBps": round(text_bytes / med["emit1"] / 1e6, 1)})
        for v in (0, 1):
            col = med[f"measure{v}"] + med["cumsum"] + med[f"emit{v}"]
            rec[f"unescape_v{v}_ms"] = round(col, 3)
            rec[f"unescape_v{v}_over_gather"] = round(col / med["gather"], 2)
            rec[f"unescape_v{v}_over_csv_text"] = round(col / med["csv_text"], 2)
    emit(rec, a.out)


def e2e_phase(torch, name, size, a):
    from alluxio_amd.minicluster import LocalAlluxioCluster
    from alluxio_amd.models import DeviceBatchLoader, IndexedRecordDataset, read_json_columns
    conf = {"alluxio.worker.tieredstore.level0.dirs.path": "hbm:0",
            "alluxio.worker.tieredstore.level0.dirs.quota": str(size + (512 << 20)),
            "alluxio.worker.hbm.page.size": "64KB",
            "alluxio.user.block.size.bytes.default": "64MB"}
    bs = 65536 if name == "scalars" else 4096
    objs = (scalar_objects if name == "scalars" else text_objects)(bs, 11)
    chunk = b"".join(as_jsonl(objs))
    columns = ({"id": ("id", "int64"), "count": ("count", "int32"), "score": ("score", "float64"), "ratio": ("ratio", "float32"),
                "ok": ("ok", "bool"), "label": ("label", "text")} if name == "scalars"
               else {"id": ("id", "int64"), "text": ("text", "text")})
    with LocalAlluxioCluster(num_workers=1, conf=conf) as c:
        fs = c.client()
        written = 0
        with fs.create_file("/json/e2e.jsonl", write_type="MUST_CACHE") as f:
            while written + len(chunk) <= size:
                f.write(chunk)
                written += len(chunk)
        dev_ms, got = [], None
        for it in range(a.e2e_rounds + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            got = read_json_columns(fs, "/json/e2e.jsonl", columns, batch_size=bs, device="cuda")
            torch.cuda.synchronize()
            if it:
                dev_ms.append((time.perf_counter() - t) * 1e3)
        ids = got["id"].values.cpu().numpy()
        last = got[len(columns) - 1]
        cuts, packed = last.offsets.cpu().numpy(), last.data.cpu().numpy().tobytes()
        key = list(columns)[-1]
        ds = IndexedRecordDataset.from_delimited(fs, "/json/e2e.jsonl", device="cuda")
        host_s, host_bytes, nb, same = 0.0, 0, 0, True
        with DeviceBatchLoader(ds, batch_size=bs, device="cuda", align=1) as dl:
            for batch in dl:
                t = time.perf_counter()
                data, off, ln = (x.cpu().numpy() for x in batch)
                buf = data.tobytes()
                rows = [json.loads(buf[int(o):int(o) + int(k)]) for o, k in zip(off[:-1], ln)]
                host_s += time.perf_counter() - t
                lo = nb * bs
                same = same and [r["id"] for r in rows] == ids[lo:lo + len(rows)].tolist()
                same = same and [r[key].encode() for r in rows] == [packed[cuts[lo + j]:cuts[lo + j + 1]] for j in range(len(rows))]
                host_bytes += int(ln.sum())
                nb += 1
                if nb >= a.host_batches:
                    break
        dev_rate = written / spread(dev_ms)["median"] / 1e6
        host_rate = host_bytes / host_s / 1e9
        emit({"what": "end_to_end", "workload": name, "file_mib": written >> 20, "rows": got.rows, "batch": bs,
              "read_json_columns_ms": spread(dev_ms, 1), "device_GBps": round(dev_rate, 3), "host_json_loads_batches": nb,
              "host_json_loads_GBps": round(host_rate, 4), "speedup": round(dev_rate / host_rate, 1),
              "equal_on_host_batches": same}, a.out)
        fs.close()
        if not same:
            raise SystemExit("the device columns and json.loads differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="scalars,text")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e-mib", type=int, default=128, help="file of the end-to-end phase (0: skip)")
    ap.add_argument("--e2e-rounds", type=int, default=3)
    ap.add_argument("--host-batches", type=int, default=2, help="batches json.loads reads")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("json_fields_bench needs a GPU: none is visible")
    from alluxio_amd.ops.native import lib
    C = lib()
    if a.out and os.path.exists(a.out):
        os.remove(a.out)
    emit({"what": "setup", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup,
          "default_fields_variant": C.json_fields_variant(), "default_text_variant": C.json_text_variant()}, a.out)
    for name in a.workloads.split(","):
        batch = 65536 if name == "scalars" else 4096
        objs = (scalar_objects if name == "scalars" else text_objects)(batch, 5)
        kernel_phase(torch, C, name, objs, batch, a)
    if a.e2e_mib:
        for name in a.workloads.split(","):
            e2e_phase(torch, name, a.e2e_mib << 20, a)


if __name__ == "__main__":
    main()
