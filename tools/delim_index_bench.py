"""Delimiter index on the GPU: kernel rate, the read-once roof, and the end-to-end call against
the stream fallback.

Per file size (``--sizes``, MiB; 128 is cache-resident, 16384 HBM-resident) and mean line length
(``--lines``, bytes), from one process:

(a) kernels: ``delim_index_raw(times=True)`` over a device arena of random text behind a scrambled
    64 KiB page table.  Device events bracket the count, scan and emit launches of each call; the
    rate is file bytes per second of their sum.  Rounds alternate A/B between the two load
    variants at the default tile, then between tile sizes with the better variant.
(b) roof: the project's CRC32C kernel (``crc32c_device``, 2 MiB pieces) over the same bytes between
    device events.  The index reads every byte twice, so the read-once roof is twice that time.
(c) end to end (``--e2e-mib``): ``build_delimited_index`` on an HBM-tier cluster against
    ``device_plan=False`` (client stream + numpy) on the same file, by the host clock.

The result of every (a) configuration is compared with numpy (``--check-mib`` and below) or, for
larger files, with a device-side count of the delimiter plus a strict-ascent check.  One JSON line
per measurement goes to stdout and to ``--out``.  Needs a GPU: it fails without one.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAGE = 64 << 10
DELIM = 0x0A
GEN = 256 << 20


def spread(xs, nd=2):
    xs = sorted(xs)
    return {"min": round(xs[0], nd), "median": round(xs[len(xs) // 2], nd), "max": round(xs[-1], nd), "n": len(xs)}


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def fill_text(torch, arena, line_len, seed):
    """Random bytes with a newline about every line_len bytes (geometric line lengths)."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    count = 0
    for s in range(0, arena.numel(), GEN):
        part = arena[s:s + GEN]
        part.view(torch.int64).random_(generator=g)
        part[part == DELIM] = 0x20
        part[torch.rand(part.numel(), device="cuda", generator=g) < 1.0 / line_len] = DELIM
        count += int((part == DELIM).sum().item())
    return count


def kernel_phase(torch, C, size, line_len, a):
    npages = size // PAGE
    arena = torch.empty(npages * PAGE, dtype=torch.uint8, device="cuda")
    in_arena = fill_text(torch, arena, line_len, seed=line_len)
    pages = np.random.default_rng(1).permutation(npages).astype(np.int64)
    plist = pages.tolist()
    nbytes = size - 12345                               # the file ends inside its last page
    last = arena[int(pages[-1]) * PAGE:][:PAGE]
    want_n = in_arena - int((last[PAGE - 12345:] == DELIM).sum().item())
    want = None
    if size <= a.check_mib << 20:
        virt = arena.cpu().numpy().reshape(npages, PAGE)[pages].reshape(-1)[:nbytes]
        want = (np.flatnonzero(virt == DELIM) + 1).astype(np.uint64)
        assert want.size == want_n
    default_variant, default_shift = C.delim_index_variant(), C.delim_index_tile_shift()

    def call(variant, shift):
        C.set_delim_index_variant(variant, shift)
        t = time.perf_counter()
        cuts, ms = C.delim_index_raw(arena.data_ptr(), plist, PAGE, 0, 0, nbytes, DELIM, 0, True)
        wall = time.perf_counter() - t
        return cuts, ms, wall

    checked = set()

    def measure(variant, shift, store):
        cuts, ms, wall = call(variant, shift)
        if (variant, shift) not in checked:
            checked.add((variant, shift))
            ok = np.array_equal(cuts, want) if want is not None else (
                cuts.size == want_n and bool((np.diff(cuts.view(np.int64)) > 0).all()) and int(cuts[-1]) <= nbytes)
            if not ok:
                raise SystemExit(f"wrong index: variant {variant} tile_shift {shift} size {size}")
        store.append((nbytes / (sum(ms) * 1e-3) / 1e9, ms, wall))

    rounds = a.rounds if size <= 1 << 30 else max(3, a.rounds // 3)
    for v in (0, 1):
        call(v, default_shift)                          # warm both code objects
    ab = {0: [], 1: []}
    for _ in range(rounds):
        for v in (0, 1):                                # A/B/A/B
            measure(v, default_shift, ab[v])
    for v in (0, 1):
        rates = [x[0] for x in ab[v]]
        emit({"what": "kernels", "size_mib": size >> 20, "line_len": line_len, "cuts": want_n, "variant": v,
              "tile_bytes": 1 << default_shift, "GBps": spread(rates),
              "count_ms": spread([x[1][0] for x in ab[v]], 3), "scan_ms": spread([x[1][1] for x in ab[v]], 3),
              "emit_ms": spread([x[1][2] for x in ab[v]], 3),
              "call_wall_ms": spread([x[2] * 1e3 for x in ab[v]], 1)}, a.out)
    best = 0 if spread([x[0] for x in ab[0]])["median"] >= spread([x[0] for x in ab[1]])["median"] else 1
    sweep = {sh: [] for sh in a.shifts}
    for _ in range(rounds):
        for sh in sweep:
            measure(best, sh, sweep[sh])
    for sh, xs in sweep.items():
        emit({"what": "tile_sweep", "size_mib": size >> 20, "line_len": line_len, "variant": best,
              "tile_bytes": 1 << sh, "GBps": spread([x[0] for x in xs]),
              "count_ms": spread([x[1][0] for x in xs], 3), "emit_ms": spread([x[1][2] for x in xs], 3)}, a.out)
    C.set_delim_index_variant(default_variant, default_shift)

    # the read-once roof: CRC32C of the same bytes, same process
    crc = []
    for it in range(rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        C.crc32c_device(arena.data_ptr(), nbytes, 2 << 20, 0)
        e1.record()
        e1.synchronize()
        if it:
            crc.append(e0.elapsed_time(e1))
    crc_ms = spread(crc, 3)
    total_ms = spread([sum(x[1]) for x in ab[best]], 3)
    emit({"what": "roof", "size_mib": size >> 20, "line_len": line_len, "crc32c_ms": crc_ms,
          "crc32c_GBps": round(nbytes / (crc_ms["median"] * 1e-3) / 1e9, 1), "index_ms": total_ms,
          "index_over_two_crc_passes": round(total_ms["median"] / (2 * crc_ms["median"]), 3)}, a.out)
    del arena
    torch.cuda.empty_cache()


def e2e_phase(torch, size, line_len, a):
    from alluxio_amd.minicluster import LocalAlluxioCluster
    from alluxio_amd.models import build_delimited_index
    conf = {"alluxio.worker.tieredstore.level0.dirs.path": "hbm:0",
            "alluxio.worker.tieredstore.level0.dirs.quota": str(size + (512 << 20)),
            "alluxio.worker.hbm.page.size": "64KB",
            "alluxio.user.block.size.bytes.default": "64MB"}
    rng = np.random.default_rng(7)
    chunk = rng.integers(0, 256, 64 << 20, dtype=np.uint8)
    chunk[chunk == DELIM] = 0x20
    chunk[rng.random(chunk.size) < 1.0 / line_len] = DELIM
    with LocalAlluxioCluster(num_workers=1, conf=conf) as c:
        fs = c.client()
        with fs.create_file("/text/e2e.jsonl", write_type="MUST_CACHE") as f:
            left = size - 12345
            while left:
                n = min(left, len(chunk))
                f.write(chunk[:n])
                left -= n
        res = {"auto": [], False: []}
        first = {}
        for it in range(a.e2e_rounds + 1):
            for plan in ("auto", False):                # A/B/A/B
                t = time.perf_counter()
                off = build_delimited_index(fs, "/text/e2e.jsonl", device_plan=plan)
                dt = time.perf_counter() - t
                first.setdefault(plan, off)
                if it:
                    res[plan].append(dt * 1e3)
        same = bool(np.array_equal(first["auto"], first[False]))
        emit({"what": "end_to_end", "size_mib": size >> 20, "line_len": line_len, "records": int(first["auto"].size - 1),
              "device_ms": spread(res["auto"], 1), "stream_numpy_ms": spread(res[False], 1), "equal": same,
              "speedup": round(spread(res[False])["median"] / spread(res["auto"])["median"], 1)}, a.out)
        if not same:
            raise SystemExit("the device index and the stream index differ")
        fs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,16384", help="file sizes in MiB")
    ap.add_argument("--lines", default="100,4096", help="mean line lengths in bytes")
    ap.add_argument("--shifts", default="13,14,15,16,17,18", help="log2 tile sizes of the sweep")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--check-mib", type=int, default=1024, help="compare with numpy up to this size")
    ap.add_argument("--e2e-mib", type=int, default=1024, help="file of the end-to-end phase (0: skip)")
    ap.add_argument("--e2e-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.shifts = [int(s) for s in a.shifts.split(",")]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("delim_index_bench needs a GPU: none is visible")
    from alluxio_amd.ops.native import lib
    C = lib()
    if a.out and os.path.exists(a.out):
        os.remove(a.out)
    emit({"what": "setup", "device": torch.cuda.get_device_name(0), "page": PAGE, "rounds": a.rounds,
          "default_tile_bytes": 1 << C.delim_index_tile_shift()}, a.out)
    for size in (int(s) << 20 for s in a.sizes.split(",")):
        for line_len in (int(x) for x in a.lines.split(",")):
            kernel_phase(torch, C, size, line_len, a)
    if a.e2e_mib:
        for line_len in (int(x) for x in a.lines.split(",")):
            e2e_phase(torch, a.e2e_mib << 20, line_len, a)


if __name__ == "__main__":
    main()
