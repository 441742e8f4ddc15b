#!/usr/bin/env python3
"""Top-K recommendation (orx_recommend_topk) at evaluation scale: 1 000 users x 1 M items x dim 64 with 200 excluded items
per user, k in {10, 100, 1000}, each kind; the yardstick in the same process (the scorer's [n, items] matrix via
score_all_items(device=True), then torch.topk); and 100 000 users at k = 100.  Kernel time from dispatch-attached events (every
launch of a call sits in the ORX_K_GEMM slot); prints one JSON line per measurement with user-item pairs/s and the fraction
of the fp32 MFMA rate (2 D flops per pair against 155 TF/s).
    python scripts/topk_bench.py [--items 1000000] [--dim 64] [--excl 200] [--reps 3] [--only a|b|c]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MFMA_FP32_TFLOPS = 155.0


def line(part, kind, users, items, dim, k, kernel_ms, wall_ms, extra=None):
    pairs = users * items
    d = {"part": part, "kind": kind, "users": users, "items": items, "dim": dim, "k": k,
         "kernel_ms": kernel_ms, "wall_ms": wall_ms, "pairs_per_s": pairs / (kernel_ms * 1e-3),
         "mfma_frac": 2.0 * dim * pairs / (kernel_ms * 1e-3) / (MFMA_FP32_TFLOPS * 1e12),
         "mfma_floor_ms": 2.0 * dim * pairs / (MFMA_FP32_TFLOPS * 1e12) * 1e3}
    d.update(extra or {})
    print(json.dumps(d), flush=True)


def timed(ctx, fn, reps):
    fn()                                                  # warm-up (buffers, first-launch attributes)
    ctx.prof_reset(); ctx.prof_enable(True)
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    wall = (time.perf_counter() - t0) / reps * 1e3
    ctx.prof_enable(False)
    p = ctx.prof_get()["gemm"]
    return p["total_ms"] / reps, wall, p["launches"] / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--excl", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="abc")
    args = ap.parse_args()
    import torch
    from openrec_amd import runtime as rt
    ctx = rt.default_context()
    NU, NI, D = 200_000, args.items, args.dim
    U = rt.Table(NU, D, ctx).init_uniform(seed=0); V = rt.Table(NI, D, ctx).init_uniform(seed=1)
    b = rt.Table(NI, 1, ctx).init_uniform(seed=2); w = rt.Table(D, 1, ctx).init_uniform(seed=3)
    rng = np.random.default_rng(0)
    uid = rng.integers(0, NU, 1000).astype(np.int32)
    excl = rt.SparseMask.from_lists([rng.choice(NI, args.excl, replace=False) for _ in range(uid.size)], NI)
    for kind in ("dot", "l2", "gmf"):
        for k in (10, 100, 1000):
            if "a" in args.only:
                ms, wall, launches, _ = timed(ctx, lambda: rt.recommend_topk(kind, U, V, b, uid, k, excl=excl, w=w), args.reps)
                line("a", kind, uid.size, NI, D, k, ms, wall, {"route": "fused (recommend_topk)", "launches": launches,
                                                               "excluded_per_user": args.excl})
            if "b" in args.only:
                # the yardstick: the score matrix, then torch.topk over it (no exclusion; its time from torch's events)
                ms_s, wall_s, _, ds = timed(ctx, lambda: rt.score_all_items(kind, U, V, b, uid, w=w, device=True), args.reps)
                torch.topk(ds.tensor, k, dim=1)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    torch.topk(ds.tensor, k, dim=1)
                e1.record(); torch.cuda.synchronize()
                ms_t = e0.elapsed_time(e1) / args.reps
                line("b", kind, uid.size, NI, D, k, ms_s + ms_t, wall_s, {"route": "score_all_items(device=True) + torch.topk",
                                                                            "score_ms": ms_s, "torch_topk_ms": ms_t})
                del ds
                torch.cuda.empty_cache()
    if "c" in args.only:
        big = np.arange(100_000, dtype=np.int32)
        ms, wall, launches, out = timed(ctx, lambda: rt.recommend_topk("dot", U, V, b, big, 100), 1)
        line("c", "dot", big.size, NI, D, 100, ms, wall, {"route": "fused (recommend_topk)", "launches": launches,
                                                         "score_matrix_gb_avoided": big.size * NI * 4 / 1e9})


if __name__ == "__main__":
    main()
