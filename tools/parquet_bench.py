"""Parquet columns on the GPU: the passes of ``read_parquet_columns`` in both variants of the hybrid
decode, the decode against the gather that fetched the same chunks, and a cached file end to end
against ``pyarrow`` on the host.

Two shapes, written by pyarrow from a seed, each one row group of 65,536 rows: ``numeric`` (eight
numeric columns: int64 and int32 with and without nulls, float64, float32, a bool, a low-cardinality
int64 that is dictionary-coded) and ``strings`` (one string column with 1,000 distinct 12-byte
values, null every 17th row, read as text and as a category).  Each is measured uncompressed and as
LZ4_RAW, from one process:

(a) passes: the file is cached on an HBM-tier cluster and read with ``read_parquet_columns``; the
    module's pass functions (page walk, LZ4, hybrid decode, place, byte-array walk, text packing,
    dictionary encode) and the loader's gather are wrapped so that each call is bracketed by a
    device synchronise and the host clock.  A pass's time is therefore what the caller waits for:
    launches, the scans between them and the small readbacks included.  The two variants alternate
    inside a round.
(b) decode against gather: the sum of the passes against the gather's time, per round.
(c) end to end (``--e2e-mib``): a cached file of about that size with the numeric columns and the
    string column, ``read_parquet_columns`` against ``pq.read_table`` on the bytes read through the
    client stream plus ``.to(device)`` of every column (strings as their dictionary codes), by the
    host clock around a device synchronise.  The host side never touches the code under test.

(d) pruning (``--prune-groups N``, alone: the other phases are skipped): a cached file of N row
    groups of ``--rows`` rows of the numeric columns plus a sorted int64 key, written by pyarrow
    with statistics; ``read_parquet_columns`` with a filter on the key that keeps one row group
    against the same read without a filter, alternating, by the host clock around a device
    synchronise, with the bytes the gather fetched and the decode launches of each.

Before timing, every column is compared with ``pq.read_table``.  One JSON line per measurement goes
to stdout and to ``--out``.  Needs a GPU: it fails without one.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PASSES = ["gather", "walk", "lz4", "hybrid", "place", "bytes", "text", "encode"]


def spread(xs, nd=3):
    xs = sorted(xs)
    return {"min": round(xs[0], nd), "median": round(xs[len(xs) // 2], nd), "max": round(xs[-1], nd), "n": len(xs)}


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def numeric_table(pa, n, seed):
    rng = np.random.default_rng(seed)
    nulls = rng.random(n) < 0.09
    return pa.table({
        "a": pa.array(rng.integers(-2 ** 62, 2 ** 62, n), pa.int64()),
        "b": pa.array(rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32), pa.int32()),
        "c": pa.array(rng.integers(-2 ** 62, 2 ** 62, n), pa.int64(), mask=nulls),
        "d": pa.array(rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32), pa.int32(), mask=nulls),
        "e": pa.array(rng.standard_normal(n), pa.float64()),
        "f": pa.array(rng.standard_normal(n).astype(np.float32), pa.float32()),
        "g": pa.array(rng.integers(0, 2, n).astype(bool), pa.bool_(), mask=nulls),
        "h": pa.array(rng.integers(0, 500, n) * 1000003, pa.int64())})


def string_table(pa, n, seed):
    rng = np.random.default_rng(seed)
    vocab = np.array([f"v{i:05d}-{(i * 7919) % 100000:05d}" for i in range(1000)])
    vals = vocab[rng.integers(0, 1000, n)]
    return pa.table({"s": pa.array(vals, pa.string(), mask=np.arange(n) % 17 == 2)})


def write(pq, tbl, lz4, rows_per_group):
    buf = io.BytesIO()
    pq.write_table(tbl, buf, compression="lz4" if lz4 else "none", row_group_size=rows_per_group)
    return buf.getvalue()


def compare(got, want, cats=()):
    for k in want.column_names:
        w = want[k].to_pylist()
        if k in cats:
            vocab = got[k].dictionary.tolist()
            g = [None if c < 0 else vocab[c].decode() for c in got[k].values.cpu().tolist()]
        else:
            g = got[k].tolist()
            if g and isinstance(next((x for x in g if x is not None), None), bytes):
                g = [None if x is None else x.decode() for x in g]
        if k in ("e", "f"):
            ok = np.array_equal(np.array(g, dtype=np.float64).view(np.int64), np.array(w, dtype=np.float64).view(np.int64))
        else:
            ok = g == w
        if not ok:
            raise SystemExit(f"column {k} differs from pq.read_table")


class PassTimer:
    """Wraps the pass functions of models.parquet (and what they call in models.fields) and the
    loader's gather; ``times`` accumulates seconds per pass between ``reset`` calls."""

    def __init__(self, sync):
        from alluxio_amd.models import dataset, fields, parquet
        self.sync, self.times, self.saved = sync, {}, []
        for mod, name, key in ((parquet, "parquet_page_table", "walk"), (parquet, "_decompress", "lz4"),
                               (parquet, "_hybrid", "hybrid"), (parquet, "_place", "place"),
                               (parquet, "_byte_spans", "bytes"), (parquet, "extract_text", "text"),
                               (fields.TextDictionary, "encode", "encode"), (dataset.DeviceBatchLoader, "gather", "gather")):
            fn = getattr(mod, name)
            self.saved.append((mod, name, fn))
            setattr(mod, name, self.wrap(fn, key))

    def wrap(self, fn, key):
        def timed(*a, **kw):
            self.sync()
            t0 = time.perf_counter()
            out = fn(*a, **kw)
            self.sync()
            self.times[key] = self.times.get(key, 0.0) + time.perf_counter() - t0
            return out
        return timed

    def reset(self):
        self.times = {}

    def restore(self):
        for mod, name, fn in self.saved:
            setattr(mod, name, fn)


@contextlib.contextmanager
def cluster(quota, device):
    from alluxio_amd.minicluster import LocalAlluxioCluster
    conf = {"alluxio.worker.tieredstore.level0.dirs.path": "hbm:0" if device == "cuda" else "dram", "alluxio.worker.tieredstore.level0.dirs.quota": quota,
            "alluxio.worker.hbm.page.size": "1MB", "alluxio.user.block.size.bytes.default": "64MB"}
    with LocalAlluxioCluster(num_workers=1, conf=conf, grpc=False) as c:
        yield c


def pass_phase(torch, C, fs, a):
    import pyarrow as pa
    import pyarrow.parquet as pq

    from alluxio_amd.models import read_parquet_columns
    shapes = {"numeric": (numeric_table(pa, a.rows, 1), None), "strings": (string_table(pa, a.rows, 2), {"s": ("s", "text"), "c": ("s", "category")})}
    default = C.parquet_decode_variant()
    for shape, (tbl, cols) in shapes.items():
        for lz4 in (False, True):
            blob = write(pq, tbl, lz4, a.rows)
            path = f"/bench/{shape}-{int(lz4)}.parquet"
            fs.write_file(path, blob, write_type="MUST_CACHE")
            want = pq.read_table(io.BytesIO(blob))
            for v in (0, 1):
                C.set_parquet_decode_variant(v)
                got = read_parquet_columns(fs, path, cols, device=a.device)
                if cols:
                    compare(got, want.rename_columns(["s"]))
                    compare(got, want.rename_columns(["c"]), cats=("c",))
                else:
                    compare(got, want)
            timer = PassTimer(a.sync)
            rounds = {0: [], 1: []}
            try:
                for r in range(a.warmup + a.rounds):
                    for v in ((0, 1) if r % 2 == 0 else (1, 0)):
                        C.set_parquet_decode_variant(v)
                        timer.reset()
                        read_parquet_columns(fs, path, cols, device=a.device)
                        if r >= a.warmup:
                            rounds[v].append(dict(timer.times))
            finally:
                timer.restore()
                C.set_parquet_decode_variant(default)
            for v in (0, 1):
                rec = {"phase": "passes", "shape": shape, "codec": "LZ4_RAW" if lz4 else "UNCOMPRESSED", "variant": v,
                       "rows": a.rows, "file_bytes": len(blob), "unit": "ms"}
                for p in PASSES:
                    xs = [1e3 * t.get(p, 0.0) for t in rounds[v]]
                    if any(xs):
                        rec[p] = spread(xs)
                dec = [1e3 * sum(t.get(p, 0.0) for p in PASSES if p != "gather") for t in rounds[v]]
                rec["decode"] = spread(dec)
                rec["decode_over_gather"] = spread([d / (1e3 * t["gather"]) for d, t in zip(dec, rounds[v])], 2)
                emit(rec, a.out)


def e2e_phase(torch, fs, a):
    import pyarrow as pa
    import pyarrow.parquet as pq

    from alluxio_amd.models import read_parquet_columns
    per_row = 8 + 4 + 8 + 4 + 8 + 4 + 1 + 2 + 14
    n = max(a.rows, (a.e2e_mib << 20) // per_row)
    num, st = numeric_table(pa, n, 5), string_table(pa, n, 6)
    tbl = num.append_column("s", st["s"])
    for lz4 in (False, True):
        blob = write(pq, tbl, lz4, a.rows)
        path = f"/bench/e2e-{int(lz4)}.parquet"
        fs.write_file(path, blob, write_type="MUST_CACHE")
        cols = {k: (k, None) for k in num.column_names}
        cols["s"] = ("s", "category")

        def ours():
            got = read_parquet_columns(fs, path, cols, device=a.device)
            a.sync()
            return got

        def host():
            with fs.open_file(path) as f:
                raw = f.read()
            t = pq.read_table(io.BytesIO(raw), read_dictionary=["s"])
            out = []
            for k in t.column_names:
                col = t[k].combine_chunks()
                if k == "s":
                    arr = col.indices.to_numpy(zero_copy_only=False)
                else:
                    arr = col.to_numpy(zero_copy_only=False)
                arr = np.ascontiguousarray(arr)
                if arr.dtype == object:
                    arr = arr.astype(np.float64)
                out.append(torch.from_numpy(arr.copy() if not arr.flags.writeable else arr).to(a.device))
            a.sync()
            return out

        got = ours()
        want = pq.read_table(io.BytesIO(blob))
        head = want.slice(0, 5000)
        for k in num.column_names:
            g = got[k].values[:5000].cpu().numpy()
            w = head[k].to_pylist()
            ok = [None if s else x for x, s in zip(g.tolist(), got[k].status[:5000].cpu().tolist())]
            if k in ("e", "f"):
                if not np.array_equal(np.array(ok, dtype=np.float64).view(np.int64), np.array(w, dtype=np.float64).view(np.int64)):
                    raise SystemExit(f"e2e column {k} differs")
            elif ok != w:
                raise SystemExit(f"e2e column {k} differs")
        host()
        t_ours, t_host = [], []
        for _ in range(a.e2e_rounds):
            for fn, acc in ((ours, t_ours), (host, t_host)):
                t0 = time.perf_counter()
                fn()
                acc.append(time.perf_counter() - t0)
        mib = len(blob) / 2 ** 20
        emit({"phase": "e2e", "codec": "LZ4_RAW" if lz4 else "UNCOMPRESSED", "rows": n, "file_mib": round(mib, 1),
              "row_groups": -(-n // a.rows), "device_ms": spread([1e3 * t for t in t_ours], 1),
              "host_pyarrow_ms": spread([1e3 * t for t in t_host], 1),
              "device_mib_s": spread([mib / t for t in t_ours], 0), "host_mib_s": spread([mib / t for t in t_host], 0),
              "speedup": spread([h / o for h, o in zip(t_host, t_ours)], 2)}, a.out)


def prune_phase(torch, C, fs, a):
    import pyarrow as pa
    import pyarrow.parquet as pq

    from alluxio_amd.models import dataset, parquet_matching_row_groups, read_parquet_columns
    n = a.prune_groups * a.rows
    tbl = numeric_table(pa, n, 7).append_column("key", pa.array(np.arange(n, dtype=np.int64) * 3, pa.int64()))
    blob = write(pq, tbl, False, a.rows)
    path = "/bench/prune.parquet"
    fs.write_file(path, blob, write_type="MUST_CACHE")
    keep = a.prune_groups // 2
    lo, hi = keep * a.rows * 3, (keep + 1) * a.rows * 3
    filt = [("key", ">=", lo), ("key", "<", hi)]
    if parquet_matching_row_groups(fs, path, filt) != [keep]:
        raise SystemExit("the filter does not keep exactly one row group")
    got = read_parquet_columns(fs, path, filters=filt, device=a.device)
    compare(got, tbl.slice(keep * a.rows, a.rows))
    fetched = [0]
    gather = dataset.DeviceBatchLoader.gather

    def counted(self, records):
        batch = gather(self, records)
        fetched[0] += int(batch.lengths.sum())
        return batch

    def read(filters):
        fetched[0] = 0
        before = C.parquet_decode_launches()
        a.sync()
        t0 = time.perf_counter()
        read_parquet_columns(fs, path, filters=filters, device=a.device)
        a.sync()
        return 1e3 * (time.perf_counter() - t0), fetched[0], C.parquet_decode_launches() - before

    dataset.DeviceBatchLoader.gather = counted
    try:
        runs = {"filtered": [], "all": []}
        for r in range(a.warmup + a.rounds):
            for name in (("filtered", "all") if r % 2 == 0 else ("all", "filtered")):
                out = read(filt if name == "filtered" else None)
                if r >= a.warmup:
                    runs[name].append(out)
    finally:
        dataset.DeviceBatchLoader.gather = gather
    rec = {"phase": "prune", "row_groups": a.prune_groups, "rows_per_group": a.rows, "file_bytes": len(blob), "unit": "ms"}
    for name, xs in runs.items():
        rec[name] = {"ms": spread([x[0] for x in xs]), "gathered_bytes": xs[0][1], "decode_launches": xs[0][2]}
    rec["filtered_over_all"] = spread([f[0] / g[0] for f, g in zip(runs["filtered"], runs["all"])], 3)
    emit(rec, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--e2e-mib", type=int, default=100)
    ap.add_argument("--e2e-rounds", type=int, default=3)
    ap.add_argument("--prune-groups", type=int, default=0,
                    help="only the pruning phase: a file of this many row groups, a filter that keeps one")
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", default="cuda", choices=["cuda", "cpu"],
                    help="cpu: a DRAM-tier cluster and the host loops (a dry run of the tool; variants do not apply)")
    a = ap.parse_args()
    import torch

    from alluxio_amd.ops.native import lib
    if a.device == "cuda" and not torch.cuda.is_available():
        raise SystemExit("parquet_bench needs a GPU")
    a.sync = torch.cuda.synchronize if a.device == "cuda" else (lambda: None)
    C = lib()
    with cluster("2GB", a.device) as c:
        fs = c.client()
        if a.prune_groups:
            prune_phase(torch, C, fs, a)
        else:
            pass_phase(torch, C, fs, a)
            if a.e2e_mib:
                e2e_phase(torch, fs, a)
        fs.close()


if __name__ == "__main__":
    main()
