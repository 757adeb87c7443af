"""Parquet pages encoded on the GPU: what ``write_parquet_columns`` costs per row group, against
the copy kernel moving the same bytes, and end to end into the cache against ``pyarrow`` on the host.

The shapes are those of ``tools/parquet_bench.py``, each one row group of 65,536 rows: ``numeric``
(eight numeric columns) and one string column of 1,000 distinct 12-byte values, as ``text`` and as
``category``.  The columns are made by ``read_parquet_columns`` from a file that pyarrow wrote from
a seed, so they lie on the device as a training loop has them.  From one process:

(a) encode: measure (with its readback), layout (the host: sizes, page headers) and emit (the scans,
    the uploads and the emit launches), everything the caller waits for before the bytes can go to
    the output stream.  Device events around the whole, ending in a synchronise, and the host clock
    around each pass with a synchronise after it for the breakdown.
(b) the roof: the batched copy kernel moving as many bytes as the row group has, in the same rounds,
    and the encode time as a multiple of it.
(c) end to end into the cache: ``write_parquet_columns`` against copying every column to the host,
    ``pa.table``, ``pq.write_table(compression="none")`` and ``fs.write_file``, alternating, by the
    host clock (both end with the file complete in the cache).

With ``--statistics`` the writer computes and writes min / max / null_count
(``statistics=True``): (a) then times the encode with and without them, alternating inside a round,
and reports the added time and the added launches (``csrc/parquet_stats.hip``) per row group; (c)
writes with them.

With ``--compression lz4_raw`` the writer compresses every page body into one LZ4 block on the
device (``csrc/lz4_block_host.h``): (a) then times the encode with and without compression,
alternating inside a round, with the compression split into parse + link (one native call), the
second readback, the host's headers and the merge; (c) writes with it, against pyarrow with
``compression="lz4"``; and two more phases follow: ``size`` (the file against pyarrow's LZ4 file
of the same table and against the host form) and ``read`` (``read_parquet_columns`` of the
compressed file against the uncompressed one, alternating).  ``--segment`` sets the segment size
for the A/B (the writer uses 32 KiB).

Before timing, the written file is compared with the source through ``pq.read_table``.  One JSON
line per measurement goes to stdout and to ``--out``.  Needs a GPU: it fails without one."""
import argparse
import io
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from parquet_bench import cluster, emit, numeric_table, spread, string_table  # noqa: E402


def host_table(pa, cols, cats=()):
    """The columns copied to the host as a pyarrow table (what a user does without the writer)."""
    out = {}
    for c in cols:
        mask = c.status.cpu().numpy() != 0
        if c.name in cats:
            words = pa.array([w.decode() for w in c.dictionary.tolist()], pa.string())
            codes = pa.array(c.values.cpu().numpy(), pa.int32(), mask=mask)
            out[c.name] = pa.DictionaryArray.from_arrays(codes, words).cast(pa.string())
        elif c.data is not None:
            valid = pa.py_buffer(np.packbits(~mask, bitorder="little"))
            out[c.name] = pa.StringArray.from_buffers(len(mask), pa.py_buffer(c.offsets.cpu().numpy().astype(np.int32)),
                                                      pa.py_buffer(c.data.cpu().numpy()), valid, int(mask.sum()))
        else:
            out[c.name] = pa.array(c.values.cpu().numpy(), mask=mask)
    return pa.table(out)


def lz4_phases(a, P, C, g, staged, shape, sync, emit_):
    """The compression of one staged row group pass by pass, by the host clock with a synchronise
    after each: parse + link (one native call, two launches), the readback of the sizes, the merge
    (with the copy of the rebuilt headers left out: the blocks go back to back)."""
    import torch
    dev = staged.device
    device, stream = P._queue(dev)
    pages, segs, scratch_bytes = P.lz4_block_tables([(b[5], b[6]) for b in g.bodies], a.segment)
    both = P._dev_i64(np.concatenate([pages.ravel(), segs.ravel()]), dev)
    scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
    result = torch.zeros(len(pages), 4, dtype=torch.int64, device=dev)
    warm = min(a.warm, 65535 - a.segment)

    def run(mode, dst=0, out=0, out_bytes=0):
        C.parquet_encode_lz4_raw(mode, staged.data_ptr(), staged.numel(), both.data_ptr(), len(pages),
                                 both[pages.size:].data_ptr(), len(segs), scratch.data_ptr(), scratch_bytes,
                                 result.data_ptr(), dst, out, out_bytes, warm, a.segment, device, stream)

    t = {"parse_link": [], "readback": [], "merge": []}
    for r in range(a.warmup + a.rounds):
        sync()
        t0 = time.perf_counter()
        run(0)
        sync()
        t1 = time.perf_counter()
        host = result.cpu().numpy()
        t2 = time.perf_counter()
        dst = np.concatenate([[0], np.cumsum(host[:, 0])]).astype(np.int64)
        d_dst = P._dev_i64(dst[:-1], dev)
        out = torch.empty(int(dst[-1]), dtype=torch.uint8, device=dev)
        sync()
        t3 = time.perf_counter()
        run(1, d_dst.data_ptr(), out.data_ptr(), out.numel())
        sync()
        t4 = time.perf_counter()
        if r >= a.warmup:
            t["parse_link"].append(1e3 * (t1 - t0))
            t["readback"].append(1e3 * (t2 - t1))
            t["merge"].append(1e3 * (t4 - t3))
    emit_({"phase": "lz4_passes", "shape": shape, "segment": a.segment, "warm": warm, "pages": len(pages), "segments": len(segs),
           "body_bytes": int(pages[:, 1].sum()), "block_bytes": int(dst[-1]), "unit": "ms",
           **{k: spread(v, 4) for k, v in t.items()}}, a.out)


def sizes_and_read(a, fs, pa, pq, cols, cats, spec, shape, sync, kw, host_table_):
    """File sizes (ours, the host form, pyarrow's LZ4 and uncompressed files of the same table) and
    read_parquet_columns of our compressed file against our uncompressed one, alternating."""
    from alluxio_amd.models import read_parquet_columns, write_parquet_columns
    from alluxio_amd.models.fields import CATEGORY, TEXT, Column, FieldColumns, TextDictionary
    write_parquet_columns(fs, "/bench/size-lz4.parquet", cols, write_type="MUST_CACHE", compression=a.compression, **kw)
    write_parquet_columns(fs, "/bench/size-plain.parquet", cols, write_type="MUST_CACHE", **kw)
    sizes = {"device_lz4_raw": fs.get_status("/bench/size-lz4.parquet").length,
             "device_uncompressed": fs.get_status("/bench/size-plain.parquet").length}
    host, dicts = [], {}
    for c in cols:                                      # the same columns on the CPU: the host form
        if c.type == TEXT:
            host.append(Column(c.name, c.field, TEXT, None, c.length.cpu(), c.status.cpu(), c.data.cpu(), c.offsets.cpu()))
        elif c.type == CATEGORY:
            d = dicts.setdefault(id(c.dictionary), TextDictionary.from_values(c.dictionary.tolist(), "cpu"))
            host.append(Column(c.name, c.field, CATEGORY, c.values.cpu(), None, c.status.cpu(), dictionary=d))
        else:
            host.append(Column(c.name, c.field, c.type, c.values.cpu(), None, c.status.cpu()))
    write_parquet_columns(fs, "/bench/size-host.parquet", FieldColumns(host), write_type="MUST_CACHE",
                          compression=a.compression, **kw)
    sizes["host_form_lz4_raw"] = fs.get_status("/bench/size-host.parquet").length
    tbl = host_table_(pa, cols, cats)
    for name, comp in (("pyarrow_lz4", "lz4"), ("pyarrow_uncompressed", "none")):
        buf = io.BytesIO()
        pq.write_table(tbl, buf, compression=comp, row_group_size=a.rows, use_dictionary=bool(cats))
        sizes[name] = len(buf.getvalue())
    emit({"phase": "size", "shape": shape, "rows": a.rows, "unit": "bytes", "segment": 32 * 1024, **sizes}, a.out)
    t_lz4, t_plain = [], []
    for r in range(a.warmup + a.rounds):
        order = (("/bench/size-lz4.parquet", t_lz4), ("/bench/size-plain.parquet", t_plain))
        for path, acc in order if r % 2 == 0 else order[::-1]:
            sync()
            t0 = time.perf_counter()
            read_parquet_columns(fs, path, spec, device=a.device)
            sync()
            if r >= a.warmup:
                acc.append(1e3 * (time.perf_counter() - t0))
    emit({"phase": "read", "shape": shape, "rows": a.rows, "unit": "ms", "lz4_raw": spread(t_lz4), "uncompressed": spread(t_plain),
          "lz4_over_uncompressed": spread([x / y for x, y in zip(t_lz4, t_plain)], 2)}, a.out)
    for p in ("/bench/size-lz4.parquet", "/bench/size-plain.parquet", "/bench/size-host.parquet"):
        fs.delete(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--statistics", action="store_true",
                    help="write statistics; the encode phase alternates with and without them")
    ap.add_argument("--compression", default=None, help="lz4_raw: compress; the encode phase alternates with and without")
    ap.add_argument("--segment", type=int, default=32 * 1024, help="bytes of a segment of the LZ4 parse (at most 61440)")
    ap.add_argument("--warm", type=int, default=4096,
                    help="bytes before a segment that its wave hashes first (segment + warm stays below 65536)")
    ap.add_argument("--device", default="cuda", choices=["cuda", "cpu"],
                    help="cpu: a DRAM-tier cluster, the host loops and the host clock (a dry run of the tool)")
    a = ap.parse_args()
    import pyarrow as pa
    import pyarrow.parquet as pq
    import torch

    from alluxio_amd.models import parquet as P
    from alluxio_amd.models import read_parquet_columns, write_parquet_columns
    from alluxio_amd.ops.native import lib
    gpu = a.device == "cuda"
    if gpu and not torch.cuda.is_available():
        raise SystemExit("parquet_write_bench needs a GPU")
    C = lib()
    sync = torch.cuda.synchronize if gpu else (lambda: None)

    class Clock:                                        # device events on the GPU, the host clock in a dry run
        def __init__(self):
            self.e = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if gpu else None

        def start(self):
            sync()
            if gpu:
                self.e[0].record()
            self.t = time.perf_counter()

        def stop(self):
            if gpu:
                self.e[1].record()
                self.e[1].synchronize()
                return self.e[0].elapsed_time(self.e[1])
            return 1e3 * (time.perf_counter() - self.t)

    shapes = {"numeric": (numeric_table(pa, a.rows, 1), None, ()),
              "text": (string_table(pa, a.rows, 2), {"s": ("s", "text")}, ()),
              "category": (string_table(pa, a.rows, 2), {"s": ("s", "category")}, ("s",))}
    kw = {"statistics": True} if a.statistics else {}   # left out otherwise: the tool also runs on a tree without them
    ckw = {"compression": a.compression} if a.compression else {}
    with cluster("2GB", a.device) as c:
        fs = c.client()
        for shape, (tbl, spec, cats) in shapes.items():
            buf = io.BytesIO()
            pq.write_table(tbl, buf, compression="none", row_group_size=a.rows)
            fs.write_file(f"/bench/{shape}-src.parquet", buf.getvalue(), write_type="MUST_CACHE")
            cols = read_parquet_columns(fs, f"/bench/{shape}-src.parquet", spec, device=a.device)
            write_parquet_columns(fs, f"/bench/{shape}-check.parquet", cols, write_type="MUST_CACHE", **kw, **ckw)
            got = pq.read_table(io.BytesIO(fs.read_file(f"/bench/{shape}-check.parquet")))
            if not got.equals(tbl.cast(got.schema)):
                raise SystemExit(f"{shape}: the written file differs from the source")
            wcols, dev = P._write_columns(cols, ())
            writer = P.ParquetWriter(fs, "/bench/unused", write_type="MUST_CACHE")
            launches = C.parquet_encode_launches()
            stats_launches = C.parquet_stats_launches() if a.statistics else 0
            g = P._measure_group(wcols, 0, a.rows, None, dev, **kw)
            P._layout_group(g, "error", writer._dict_offsets)
            staged = P._emit_group(g)
            out_bytes = int(staged.numel())
            comp_bytes = int(P._compress_group(g, staged, a.segment, a.warm)[0].numel()) if a.compression else out_bytes
            launches = C.parquet_encode_launches() - launches
            stats_launches = C.parquet_stats_launches() - stats_launches if a.statistics else 0
            src = torch.randint(0, 256, (out_bytes,), dtype=torch.uint8, device=a.device)
            dst = torch.empty_like(src)
            stream = int(torch.cuda.current_stream().cuda_stream) if gpu else 0
            clock = Clock()
            total, passes, roof, plain = [], [], [], []
            for r in range(a.warmup + a.rounds):
                def encode(kw=kw, compress=bool(a.compression)):
                    clock.start()
                    t0 = time.perf_counter()
                    g = P._measure_group(wcols, 0, a.rows, None, dev, **kw)
                    t1 = time.perf_counter()
                    P._layout_group(g, "error", writer._dict_offsets)
                    t2 = time.perf_counter()
                    staged = P._emit_group(g)
                    if compress:
                        sync()
                        t3 = time.perf_counter()
                        P._compress_group(g, staged, a.segment, a.warm)
                    ms = clock.stop()
                    t4 = time.perf_counter()
                    if not compress:
                        t3 = t4
                    return ms, {"measure": 1e3 * (t1 - t0), "layout": 1e3 * (t2 - t1), "emit": 1e3 * (t3 - t2),
                                "compress": 1e3 * (t4 - t3)}

                def copy():
                    clock.start()
                    if gpu:
                        C.batched_copy([(src.data_ptr(), dst.data_ptr(), out_bytes)], stream, False)
                    else:
                        dst.copy_(src)
                    return clock.stop()

                fns = [("encode", encode), ("copy", copy)]
                if a.statistics or a.compression:       # the same encode without either, in the same rotation
                    fns.append(("plain", lambda: encode({}, False)))
                k = r % len(fns)
                got = {name: fn() for name, fn in fns[k:] + fns[:k]}
                enc, cp = got["encode"], got["copy"]
                if r >= a.warmup:
                    if a.statistics or a.compression:
                        plain.append(got["plain"][0])
                    total.append(enc[0])
                    passes.append(enc[1])
                    roof.append(cp)
            rec = {"phase": "encode", "shape": shape, "rows": a.rows, "row_group_bytes": out_bytes, "launches": launches,
                   "unit": "ms", "encode": spread(total), "copy_kernel": spread(roof, 4),
                   "encode_over_copy": spread([t / c_ for t, c_ in zip(total, roof)], 1)}
            for k in ("measure", "layout", "emit") + (("compress",) if a.compression else ()):
                rec[k] = spread([p[k] for p in passes])
            if a.compression:
                rec.update(compression=a.compression, segment=a.segment, warm=min(a.warm, 65535 - a.segment),
                           compressed_bytes=comp_bytes,
                           encode_without=spread(plain), added=spread([t - p for t, p in zip(total, plain)]))
            if a.statistics:
                rec.pop("encode_without", None)
                rec.update(statistics=True, stats_launches=stats_launches, encode_without=spread(plain),
                           added=spread([t - p for t, p in zip(total, plain)]))
            emit(rec, a.out)
            if a.compression:
                lz4_phases(a, P, C, g, staged, shape, sync, emit)

            def ours():
                write_parquet_columns(fs, "/bench/e2e-ours.parquet", cols, write_type="MUST_CACHE", **kw, **ckw)
                fs.delete("/bench/e2e-ours.parquet")

            def host():
                buf = io.BytesIO()
                pq.write_table(host_table(pa, cols, cats), buf, compression="lz4" if a.compression else "none",
                               row_group_size=a.rows)
                fs.write_file("/bench/e2e-host.parquet", buf.getvalue(), write_type="MUST_CACHE")
                fs.delete("/bench/e2e-host.parquet")

            t_ours, t_host = [], []
            for r in range(a.warmup + a.rounds):
                for fn, acc in ((ours, t_ours), (host, t_host)) if r % 2 == 0 else ((host, t_host), (ours, t_ours)):
                    sync()
                    t0 = time.perf_counter()
                    fn()
                    sync()
                    if r >= a.warmup:
                        acc.append(1e3 * (time.perf_counter() - t0))
            emit({"phase": "e2e", "shape": shape, "rows": a.rows, "unit": "ms", "statistics": a.statistics,
                  "compression": a.compression,
                  "device_write": spread(t_ours),
                  "host_pyarrow_write": spread(t_host), "host_over_device": spread([h / o for h, o in zip(t_host, t_ours)], 2)},
                 a.out)
            if a.compression:
                sizes_and_read(a, fs, pa, pq, cols, cats, spec, shape, sync, kw, host_table)
        fs.close()


if __name__ == "__main__":
    main()
