#!/usr/bin/env python3
"""Dynamic negative sampling at training scale: `DeviceSampler.pairwise_hard` on 1 M users x 1 M items x dim 64, n = 65 536
samples per call, M in {1, 4, 8, 16} candidates, ids and tables resident.  Per M: the time of one call (host clock around a
batch of back-to-back calls that ends in a synchronise, divided by the calls; the median over the batches after a warm-up),
the algorithmic bytes n (M + 1) (4 D + 4) -- M item rows and one user row per sample, 4 bytes of id or bias with each -- and
that traffic as a fraction of the float4 copy rate `orx_copy_bandwidth` measures in the same process.  Beside it the time of
`DeviceSampler.pairwise` (the draw alone) for the same n, and per M the time `orx_table_gather` takes for n (M + 1) random item
rows on device ids (it reads every row and writes it out again).  One JSON line per measurement, all of them again in `--out`.
    python scripts/hard_neg_bench.py [--users 1000000] [--items 1000000] [--dim 64] [--n 65536] [--records 4000000] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--records", type=int, default=4_000_000)
    ap.add_argument("--calls", type=int, default=200, help="back-to-back calls per timed batch")
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--model", default="bpr", choices=["bpr", "ucml"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from openrec_amd import _ffi, runtime as rt
    NU, NI, D, n = args.users, args.items, args.dim, args.n
    rng = np.random.default_rng(0)
    raw = np.zeros(args.records, dtype=[("user_id", np.int32), ("item_id", np.int32)])
    raw["user_id"] = rng.integers(0, NU, args.records); raw["item_id"] = rng.integers(0, NI, args.records)
    ctx = rt.default_context()
    sm = rt.DeviceSampler(raw, NU, NI, ctx)
    U = rt.Table(NU, D).init_uniform(seed=0); V = rt.Table(NI, D).init_uniform(seed=1); b = rt.Table(NI, 1).init_uniform(seed=2)
    dev = torch.device("cuda", 0)
    uid, pid, nid = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    def timed(fn):
        """ms per call: median and minimum over the batches"""
        for k in range(20):
            fn(k)
        ctx.synchronize()
        per = []
        for r in range(args.batches):
            t0 = time.perf_counter()
            for k in range(args.calls):
                fn(r * args.calls + k)                       # every call another window of the stream
            ctx.synchronize()
            per.append((time.perf_counter() - t0) * 1e3 / args.calls)
        return float(np.median(per)), float(min(per))

    gbps = ctx.copy_bandwidth(1 << 30, 10)
    shape = {"users": NU, "items": NI, "dim": D, "n": n, "records": args.records, "model": args.model,
             "calls_per_batch": args.calls, "batches": args.batches}
    med, lo = timed(lambda k: sm.pairwise(5, k * n, n, uid, pid, nid))
    emit({"part": "draw", "call": "DeviceSampler.pairwise", **shape, "ms_median": med, "ms_min": lo, "copy_gbps": gbps})
    for M in (1, 4, 8, 16):
        med, lo = timed(lambda k: sm.pairwise_hard(5, k * n, n, uid, pid, nid, args.model, U, V, b, candidates=M))
        model_bytes = n * (M + 1) * (4 * D + 4)
        floor_ms = model_bytes / (gbps * 1e9) * 1e3
        emit({"part": "hard", "call": "DeviceSampler.pairwise_hard", "candidates": M, **shape, "ms_median": med, "ms_min": lo,
              "model_bytes": model_bytes, "copy_gbps": gbps, "model_ms_at_copy_rate": floor_ms, "frac_of_copy_rate": floor_ms / med,
              "rows_per_s": n * (M + 1) / (med * 1e-3)})
        rows = n * (M + 1)
        ids = torch.randint(0, NI, (rows,), dtype=torch.int32, device=dev)
        out = torch.empty(rows * D, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        med, lo = timed(lambda k: rt.check(ctx._lib.orx_table_gather(V._h, ids.data_ptr(), rows, out.data_ptr(), _ffi.ORX_IDS_DEVICE)))
        emit({"part": "gather", "call": "orx_table_gather", "rows": rows, "dim": D, "ms_median": med, "ms_min": lo,
              "rows_per_s": rows / (med * 1e-3), "read_plus_written_bytes": rows * (8 * D + 4)})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
