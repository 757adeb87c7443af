"""Text dictionaries on the GPU: ``TextDictionary.encode`` / ``lookup`` in both probe variants, what
they add to the text-column passes of the same batch, the host path they replace, and
``read_delimited_columns`` of one category column end to end.

Three workloads of 65,536 values (``--rows``), generated from a seed: ``short`` (about 12 bytes,
1,000 distinct values), ``distinct`` (about 12 bytes, every value different) and ``long`` (about
200 bytes, 1,000 distinct values).  Per workload, from one process, rounds that alternate the
candidates (``--warmup`` rounds first, then ``--rounds``), each timed by the host clock around a
device synchronise, so a call's readback is part of it:

  fill v0 / v1     a fresh dictionary and the first ``encode`` of the batch (table growth included)
  encode v0 / v1   ``encode`` of the same batch again: steady state, nothing new
  lookup v0 / v1   ``lookup`` of the batch: no readback
  text passes      ``_text_passes`` (measure, cumsum, readback, emit) over the same values as spans:
                   what a text column of this batch costs, so encode / text is what a category
                   column adds on top
  host path        the path this replaces: ``Column.tolist()``, a Python ``dict.setdefault`` loop and
                   the codes copied back to the device

Before timing, both variants and the host loops are compared with the ``setdefault`` loop.  Then
(``--e2e-mib``, 0 skips) a cached CSV file ``id,label,number`` on an HBM-tier cluster is read with
``read_delimited_columns`` once with the label as a category column and once as a text column.

One JSON line per measurement goes to stdout and to ``--out``; ``--md`` writes the table and the
choice of default variant (the faster on ``short``, ``encode`` and ``lookup`` together).  Needs a GPU: it fails without one.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

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


def workload(name, rows, seed):
    rng = np.random.default_rng(seed)
    if name == "distinct":
        return [b"user-%07d" % i for i in rng.permutation(10 * rows)[:rows]]
    size = 200 if name == "long" else 0
    pool = [b"label-%06d" % i + b"x" * max(0, size - 12 + int(k)) for i, k in
            zip(rng.permutation(10 ** 6)[:1000], rng.integers(-8, 9, 1000))]
    return [pool[i] for i in rng.integers(0, 1000, rows)]


def batch_of(torch, values, device):
    from alluxio_amd.models import RaggedBatch
    lens = np.array([len(v) for v in values], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    data = torch.from_numpy(np.frombuffer(b"".join(values), dtype=np.uint8).copy()).to(device)
    return RaggedBatch(data, torch.from_numpy(offs).to(device), torch.from_numpy(lens.astype(np.int32)).to(device))


def kernel_phase(torch, C, name, values, a):
    from alluxio_amd.models import TextDictionary
    from alluxio_amd.models.fields import TEXT, Column, _text_passes
    n = len(values)
    ref = {}
    want = [ref.setdefault(v, len(ref)) for v in values]
    batch = batch_of(torch, values, "cuda")
    start, length = batch.offsets[:n].contiguous(), batch.lengths
    for v in (0, 1):                                    # both variants and the host loops against the loop above
        C.set_text_dict_variant(v)
        d = TextDictionary("cuda")
        if d.encode(batch).cpu().tolist() != want or d.tolist() != list(ref) or d.lookup(batch).cpu().tolist() != want:
            raise SystemExit(f"{name}: variant {v} differs from the setdefault loop")
    h = TextDictionary("cpu")
    t0 = time.perf_counter()
    host_codes = h.encode(batch_of(torch, values, "cpu")).tolist()
    host_loop_ms = (time.perf_counter() - t0) * 1e3
    if host_codes != want:
        raise SystemExit(f"{name}: the host loops differ from the setdefault loop")
    warm = {}
    for v in (0, 1):
        C.set_text_dict_variant(v)
        warm[v] = TextDictionary("cuda")
        warm[v].encode(batch)
    column = Column(None, 0, TEXT, None, length, torch.zeros(n, dtype=torch.uint8, device="cuda"), batch.data,
                    batch.offsets)

    def fill(v):
        C.set_text_dict_variant(v)
        TextDictionary("cuda").encode(batch)

    def encode(v):
        C.set_text_dict_variant(v)
        warm[v].encode(batch)

    def lookup(v):
        C.set_text_dict_variant(v)
        warm[v].lookup(batch)

    def text():
        _text_passes(batch.data, [(start, length, None)], Q)

    def host():
        d = {}
        return torch.tensor([d.setdefault(x, len(d)) for x in column.tolist()], dtype=torch.int32).cuda()

    steps = [("fill_v0", lambda: fill(0)), ("fill_v1", lambda: fill(1)), ("encode_v0", lambda: encode(0)),
             ("encode_v1", lambda: encode(1)), ("lookup_v0", lambda: lookup(0)), ("lookup_v1", lambda: lookup(1)),
             ("text_passes", text), ("host_path", host)]
    times = {k: [] for k, _ in steps}
    for it in range(a.warmup + a.rounds):
        for k, fn in steps:                             # the candidates alternate inside a round
            if k == "host_path" and it >= a.warmup + a.host_rounds:
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    if host().cpu().tolist() != want:
        raise SystemExit(f"{name}: the host path differs")
    med = {k: spread(v)["median"] for k, v in times.items()}
    nbytes = int(batch.data.numel())
    rec = {"what": "dictionary", "workload": name, "rows": n, "distinct": len(ref), "value_bytes": nbytes,
           "mean_value": round(nbytes / n, 1), **{k + "_ms": spread(v) for k, v in times.items()},
           "host_loops_ms": round(host_loop_ms, 2)}
    for v in (0, 1):
        rec[f"encode_v{v}_Mvalues_per_s"] = round(n / med[f"encode_v{v}"] / 1e3, 1)
        rec[f"encode_v{v}_over_text_passes"] = round(med[f"encode_v{v}"] / med["text_passes"], 2)
        rec[f"host_path_over_encode_v{v}"] = round(med["host_path"] / med[f"encode_v{v}"], 1)
    rec["encode_v0_over_v1"] = round(med["encode_v0"] / med["encode_v1"], 2)
    rec["equal"] = True
    emit(rec, a.out)
    return rec


def e2e_phase(torch, C, size, a):
    from alluxio_amd.minicluster import LocalAlluxioCluster
    from alluxio_amd.models import read_delimited_columns
    conf = {"alluxio.worker.tieredstore.level0.dirs.path": "hbm:0",
            "alluxio.worker.tieredstore.level0.dirs.quota": str(size + (512 << 20)),
            "alluxio.worker.hbm.page.size": "64KB",
            "alluxio.user.block.size.bytes.default": "64MB"}
    labels = workload("short", 65536, 11)
    chunk = b"".join(b'%d,%s,%d\n' % (i, (b'"' + v + b'"') if i % 4 == 0 else v, i * 31) for i, v in enumerate(labels))
    with LocalAlluxioCluster(num_workers=1, conf=conf) as c:
        fs = c.client()
        written = 0
        with fs.create_file("/dict/e2e.csv", write_type="MUST_CACHE") as f:
            while written + len(chunk) <= size:
                f.write(chunk)
                written += len(chunk)
        times = {"category": [], "text": []}
        got = {}
        for it in range(a.e2e_rounds + 1):
            for kind in ("category", "text"):
                torch.cuda.synchronize()
                t = time.perf_counter()
                got[kind] = read_delimited_columns(fs, "/dict/e2e.csv", [(1, kind)], quote='"', batch_size=65536,
                                                   device="cuda")
                torch.cuda.synchronize()
                if it:
                    times[kind].append((time.perf_counter() - t) * 1e3)
        cat, text = got["category"][0], got["text"][0]
        ref = {}
        want = [ref.setdefault(v, len(ref)) for v in text.tolist()]
        same = cat.tolist() == want and cat.dictionary.tolist() == list(ref)
        mc, mt = spread(times["category"])["median"], spread(times["text"])["median"]
        emit({"what": "end_to_end", "file_mib": written >> 20, "rows": cat.values.numel(), "distinct": len(ref),
              "variant": C.text_dict_variant(), "category_ms": spread(times["category"], 1),
              "text_ms": spread(times["text"], 1), "category_GBps": round(written / mc / 1e6, 2),
              "text_GBps": round(written / mt / 1e6, 2), "category_over_text": round(mc / mt, 2), "equal": same}, a.out)
        fs.close()
        if not same:
            raise SystemExit("the category column differs from the loop over the text column")


def write_md(path, setup, recs, e2e_line, default):
    rows = ["fill_v0", "fill_v1", "encode_v0", "encode_v1", "lookup_v0", "lookup_v1", "text_passes", "host_path"]
    out = ["# Text dictionaries: measured on " + setup["device"], "",
           f"`tools/text_dict_bench.py`, {setup['rounds']} rounds after {setup['warmup']} warm-up rounds, the candidates",
           "alternating inside a round; host clock around a device synchronise; milliseconds, median (min - max).", "",
           "| call | " + " | ".join(f"{r['workload']} ({r['mean_value']} B, {r['distinct']} distinct)" for r in recs) + " |",
           "|---|" + "---|" * len(recs)]
    for k in rows:
        cells = ["{median} ({min} - {max})".format(**r[k + "_ms"]) for r in recs]
        out.append(f"| {k.replace('_', ' ')} | " + " | ".join(cells) + " |")
    for k in ("encode_v0_over_v1", "encode_v0_over_text_passes", "encode_v1_over_text_passes", "host_path_over_encode_v0",
              "host_path_over_encode_v1"):
        out.append(f"| {k.replace('_', ' ')} | " + " | ".join(str(r[k]) for r in recs) + " |")
    short = [r for r in recs if r["workload"] == "short"]
    out += ["", f"All of {recs[0]['rows']} values per batch; every result was compared with the `setdefault` loop first."]
    if short:
        s = short[0]
        both = [s[f"encode_v{v}_ms"]["median"] + s[f"lookup_v{v}_ms"]["median"] for v in (0, 1)]
        best = 0 if both[0] <= both[1] else 1
        out += ["", f"Default variant: on `short`, steady-state `encode` takes {s['encode_v0_ms']['median']} ms with v0 and "
                f"{s['encode_v1_ms']['median']} ms with v1, `lookup` {s['lookup_v0_ms']['median']} ms and "
                f"{s['lookup_v1_ms']['median']} ms; the faster of the two over both calls is variant {best}.  "
                f"The build measured here has default {default}."]
    if e2e_line:
        e = e2e_line
        out += ["", f"End to end, `read_delimited_columns` of a cached {e['file_mib']} MiB CSV ({e['rows']} rows, batches of "
                f"65,536, variant {e['variant']}): category column {e['category_ms']['median']} ms "
                f"({e['category_GBps']} GB/s of file bytes), text column {e['text_ms']['median']} ms "
                f"({e['text_GBps']} GB/s): ratio {e['category_over_text']}."]
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--workloads", default="short,distinct,long")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-rounds", type=int, default=3, help="rounds that also time the host path")
    ap.add_argument("--e2e-mib", type=int, default=64, help="file of the end-to-end phase (0: skip)")
    ap.add_argument("--e2e-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("text_dict_bench needs a GPU: none is visible")
    from alluxio_amd.ops.native import lib
    C = lib()
    if a.out and os.path.exists(a.out):
        os.remove(a.out)
    default = C.text_dict_variant()
    setup = {"what": "setup", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup,
             "default_variant": default}
    emit(setup, a.out)
    recs, e2e = [], None
    try:
        for i, name in enumerate(a.workloads.split(",")):
            recs.append(kernel_phase(torch, C, name, workload(name, a.rows, 5 + i), a))
    finally:
        C.set_text_dict_variant(default)
    if a.e2e_mib:
        e2e_phase(torch, C, a.e2e_mib << 20, a)
        if a.out:
            e2e = json.loads(open(a.out).read().splitlines()[-1])
    if a.md:
        write_md(a.md, setup, recs, e2e, default)


if __name__ == "__main__":
    main()
