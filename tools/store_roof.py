"""Store-only roof of the ring read on this GPU: a 256 MiB device buffer (one bench step's ring) is
filled with 16-B vector stores from a persistent grid and nothing is loaded, so the rate printed
here is the ceiling of the bench's headline (`local`), whose source is served by L2 and whose ring
stores are all that reaches memory.  Plain and nontemporal stores, at the persistent grid (CUs x
resident workgroups) and at explicit grids, in interleaved rounds of one process; one JSON line per
combination with the median, min and max over the rounds."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50, help="fills per timed window")
    ap.add_argument("--grids", default="0,1024,2048,4096,8192", help="0 = CUs x resident workgroups")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("store_roof needs a HIP device")
    from alluxio_amd.ops.native import lib
    C = lib()
    n = a.mib << 20
    dst = torch.empty(n, dtype=torch.uint8, device="cuda")
    stream = int(torch.cuda.current_stream().cuda_stream)
    combos = [(nt, int(g)) for nt in (False, True) for g in a.grids.split(",")]
    rates = {k: [] for k in combos}
    used = {}
    for k in combos:                                     # warm up: code objects, the occupancy query
        used[k] = C.store_fill(dst.data_ptr(), n, 0x5A5A5A5A, k[0], k[1], stream)
    torch.cuda.synchronize()
    assert bool((dst.view(torch.int32) == 0x5A5A5A5A).all())
    for _ in range(a.rounds):
        for k in combos:
            for _ in range(3):
                C.store_fill(dst.data_ptr(), n, 1, k[0], k[1], stream)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(a.iters):
                C.store_fill(dst.data_ptr(), n, 1, k[0], k[1], stream)
            torch.cuda.synchronize()
            rates[k].append(n * a.iters / (time.perf_counter() - t) / 1e12)
    rows = []
    for k in combos:
        row = {"bytes": n, "nontemporal": k[0], "grid": used[k], "rounds": a.rounds, "iters": a.iters,
               "TBps_median": round(statistics.median(rates[k]), 3), "TBps_min": round(min(rates[k]), 3),
               "TBps_max": round(max(rates[k]), 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
