"""Snappy pages on the GPU: the two decode kernels against each other, against the LZ4 decoder on
the same data and against the host, and a cached Snappy file end to end.

The shapes are those of ``tools/parquet_bench.py``: one row group of 65,536 rows (``--rows``) with
the eight numeric columns and the string column of 1,000 distinct values, written by pyarrow from a
seed with its default 1 MiB pages, as ``compression="snappy"`` and as ``compression="lz4"``.

(a) kernel: the compressed pages of the row group (found with the page walk on the host) are decoded
    straight from the file's bytes in device memory: ``snappy_device_kernel_ms`` in both variants
    and ``lz4_device_kernel_ms`` at its default variant on the LZ4_RAW form, alternating inside a
    round (HIP events around ``--reps`` launches, the chunk table uploaded once), and
    ``pa.Codec("snappy").decompress`` of the same pages on the host, for scale.  Before timing,
    every page of every variant is compared with pyarrow's bytes.
(b) end to end (``--e2e-mib``): a cached file of about that size, ``read_parquet_columns(codecs="all")``
    of the Snappy form (at the default kernel variant) against the LZ4_RAW and the uncompressed form
    and against ``pq.read_table`` of the Snappy form through the client stream plus ``.to(device)``,
    alternating, by the host clock around a device synchronise.

One JSON line per measurement goes to stdout and to ``--out``.  Needs a GPU: it fails without one
(``--device cpu`` is a dry run of the tool on a DRAM tier that times the host loops only).
"""
import argparse
import io
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from parquet_bench import cluster, emit, numeric_table, spread, string_table  # noqa: E402


def table(pa, n, seed):
    return numeric_table(pa, n, seed).append_column("s", string_table(pa, n, seed + 1)["s"])


def written(pq, tbl, compression, rows):
    buf = io.BytesIO()
    pq.write_table(tbl, buf, compression=compression, row_group_size=rows)
    return buf.getvalue()


def pages_of(torch, blob):
    """(offset, compressed bytes, uncompressed bytes) of every page of the file's first row group."""
    import pyarrow.parquet as pq

    from alluxio_amd.models import parquet_page_table
    rg = pq.ParquetFile(io.BytesIO(blob)).metadata.row_group(0)
    out = []
    for j in range(rg.num_columns):
        cc = rg.column(j)
        start = cc.dictionary_page_offset or cc.data_page_offset
        chunk = torch.from_numpy(np.frombuffer(blob[start:start + cc.total_compressed_size], dtype=np.uint8).copy())
        tab, _counts, errors = parquet_page_table(chunk, [0], [chunk.numel()])
        if errors.any():
            raise SystemExit("the page walk failed on pyarrow's file")
        for r in tab:
            if r[0] == 3:
                raise SystemExit("V1 pages expected")
            out.append((start + int(r[1]), int(r[2]), int(r[3])))
    return out


def kernel_phase(torch, C, a):
    import pyarrow as pa
    import pyarrow.parquet as pq
    tbl = table(pa, a.rows, 1)
    snappy, lz4 = pa.Codec("snappy"), pa.Codec("lz4_raw")
    forms = {}
    for name, codec in (("SNAPPY", snappy), ("LZ4_RAW", lz4)):
        blob = written(pq, tbl, "snappy" if name == "SNAPPY" else "lz4", a.rows)
        pages = pages_of(torch, blob)
        want = [codec.decompress(blob[o:o + c], decompressed_size=u, asbytes=True) for o, c, u in pages]
        forms[name] = (blob, pages, want)
    base = {"phase": "kernel", "rows": a.rows, "unit": "ms"}
    # the host, for scale
    blob, pages, want = forms["SNAPPY"]
    host = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for o, c, u in pages:
            snappy.decompress(blob[o:o + c], decompressed_size=u)
        host.append(1e3 * (time.perf_counter() - t0))
    emit(dict(base, what="host pa.Codec('snappy').decompress", pages=len(pages), compressed_bytes=sum(p[1] for p in pages),
              uncompressed_bytes=sum(p[2] for p in pages), ms=spread(host)), a.out)
    if a.device != "cuda":
        return
    runs = {}
    for name, (blob, pages, want) in forms.items():
        src = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to("cuda")
        dst_off = np.concatenate([[0], np.cumsum([(u + 15) // 16 * 16 + 16 for _o, _c, u in pages])])
        dst = torch.zeros(int(dst_off[-1]), dtype=torch.uint8, device="cuda")
        chunks = [(src.data_ptr() + o, dst.data_ptr() + int(d), c, u) for (o, c, u), d in zip(pages, dst_off)]
        variants = (0, 1) if name == "SNAPPY" else (None,)
        for v in variants:
            dst.zero_()
            if name == "SNAPPY":
                C.set_snappy_decode_variant(v)
                sizes = C.snappy_device(chunks)
            else:
                sizes = C.lz4_device(chunks, False)
            got = dst.cpu().numpy()
            for (o, c, u), d, w, s in zip(pages, dst_off, want, sizes):
                if s != u or got[int(d):int(d) + u].tobytes() != w:
                    raise SystemExit(f"{name} variant {v}: a page differs from pyarrow's bytes")
            runs[(name, v)] = (chunks, [], src, dst)
    order = list(runs)
    for r in range(a.warmup + a.rounds):
        for key in (order if r % 2 == 0 else order[::-1]):
            name, v = key
            chunks = runs[key][0]
            if name == "SNAPPY":
                C.set_snappy_decode_variant(v)
                ms = C.snappy_device_kernel_ms(chunks, a.reps)
            else:
                ms = C.lz4_device_kernel_ms(chunks, False, a.reps)
            if r >= a.warmup:
                runs[key][1].append(ms)
    C.set_snappy_decode_variant(-1)
    for (name, v), (chunks, xs, _s, _d) in runs.items():
        unc = sum(ch[3] for ch in chunks)
        emit(dict(base, what="kernel", codec=name, variant=v, pages=len(chunks), compressed_bytes=sum(ch[2] for ch in chunks),
                  uncompressed_bytes=unc, ms=spread(xs, 4), gb_s_out=spread([unc / (1e6 * x) for x in xs], 2)), a.out)


def e2e_phase(torch, fs, a):
    import pyarrow as pa
    import pyarrow.parquet as pq

    from alluxio_amd.models import read_parquet_columns
    per_row = 8 + 4 + 8 + 4 + 8 + 4 + 1 + 2 + 14
    n = max(a.rows, (a.e2e_mib << 20) // per_row)
    tbl = table(pa, n, 5)
    cols = {k: (k, None) for k in tbl.column_names if k != "s"}
    cols["s"] = ("s", "category")
    paths, sizes = {}, {}
    for name, comp in (("SNAPPY", "snappy"), ("LZ4_RAW", "lz4"), ("UNCOMPRESSED", "none")):
        blob = written(pq, tbl, comp, a.rows)
        paths[name], sizes[name] = f"/bench/e2e-{comp}.parquet", len(blob)
        fs.write_file(paths[name], blob, write_type="MUST_CACHE")

    def ours(name):
        got = read_parquet_columns(fs, paths[name], cols, device=a.device, codecs="all")
        a.sync()
        return got

    def host():
        with fs.open_file(paths["SNAPPY"]) as f:
            raw = f.read()
        t = pq.read_table(io.BytesIO(raw), read_dictionary=["s"])
        out = []
        for k in t.column_names:
            col = t[k].combine_chunks()
            arr = np.ascontiguousarray((col.indices if k == "s" else col).to_numpy(zero_copy_only=False))
            if arr.dtype == object:
                arr = arr.astype(np.float64)
            out.append(torch.from_numpy(arr.copy() if not arr.flags.writeable else arr).to(a.device))
        a.sync()
        return out

    ref = ours("UNCOMPRESSED")
    for name in ("SNAPPY", "LZ4_RAW"):
        got = ours(name)
        for k in cols:
            if not (torch.equal(got[k].values, ref[k].values) and torch.equal(got[k].status, ref[k].status)):
                raise SystemExit(f"e2e column {k} of the {name} form differs from the uncompressed form")
    head = tbl.slice(0, 5000)
    for k in ("a", "d", "h"):
        ok = [None if s else x for x, s in zip(ref[k].values[:5000].cpu().tolist(), ref[k].status[:5000].cpu().tolist())]
        if ok != head[k].to_pylist():
            raise SystemExit(f"e2e column {k} differs from the table")
    host()
    names = ["SNAPPY", "LZ4_RAW", "UNCOMPRESSED", "host"]
    times = {k: [] for k in names}
    for r in range(a.e2e_rounds):
        for k in (names if r % 2 == 0 else names[::-1]):
            t0 = time.perf_counter()
            host() if k == "host" else ours(k)
            times[k].append(1e3 * (time.perf_counter() - t0))
    emit({"phase": "e2e", "rows": n, "row_groups": -(-n // a.rows), "unit": "ms",
          "file_mib": {k: round(v / 2 ** 20, 1) for k, v in sizes.items()},
          "device_ms": {k: spread(times[k], 1) for k in names[:3]},
          "host_pyarrow_snappy_ms": spread(times["host"], 1),
          "speedup_over_host": spread([h / o for h, o in zip(times["host"], times["SNAPPY"])], 2),
          "snappy_over_lz4_raw": spread([s / l for s, l in zip(times["SNAPPY"], times["LZ4_RAW"])], 2)}, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20, help="launches per kernel timing")
    ap.add_argument("--e2e-mib", type=int, default=100)
    ap.add_argument("--e2e-rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", default="cuda", choices=["cuda", "cpu"])
    a = ap.parse_args()
    import torch

    from alluxio_amd.ops.native import lib
    if a.device == "cuda" and not torch.cuda.is_available():
        raise SystemExit("snappy_bench needs a GPU")
    a.sync = torch.cuda.synchronize if a.device == "cuda" else (lambda: None)
    C = lib()
    kernel_phase(torch, C, a)
    if a.e2e_mib:
        with cluster("2GB", a.device) as c:
            fs = c.client()
            e2e_phase(torch, fs, a)
            fs.close()


if __name__ == "__main__":
    main()
