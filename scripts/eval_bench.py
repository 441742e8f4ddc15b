#!/usr/bin/env python3
"""Evaluation without a score matrix (orx_rank_metrics_matrixfree) at evaluation scale: 1 000 users x 1 M items x dim 64 with
20 positives and 200 excluded items per user, each kind, against the materialised path (rank_metrics_csr(kind=...): the scorer's
[n, items] matrix plus the bitmap sweeps) in the same process; and 100 000 users with the default scratch budget.  Wall time
covers the whole call (both paths upload the lists and download the metrics, and return synchronised).  Kernel time from
dispatch-attached events covers the ORX_K_GEMM slot only: the matrix-free sweeps and the gather, but for the matrix path only
the scorer -- its rank sweeps carry no events -- so `gemm_ms` is a lower bound there.  One JSON line per measurement.
    python scripts/eval_bench.py [--items 1000000] [--dim 64] [--pos 20] [--excl 200] [--reps 5] [--only a|b|c]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MFMA_FP32_TFLOPS = 155.0


def line(part, kind, users, items, dim, gemm_ms, wall_ms, extra=None):
    pairs = users * items
    d = {"part": part, "kind": kind, "users": users, "items": items, "dim": dim, "gemm_ms": gemm_ms, "wall_ms": wall_ms,
         "pairs_per_s_wall": pairs / (wall_ms * 1e-3), "mfma_floor_ms": 2.0 * dim * pairs / (MFMA_FP32_TFLOPS * 1e12) * 1e3}
    d.update(extra or {})
    print(json.dumps(d), flush=True)


def timed(ctx, fn, reps, warm=2):
    for _ in range(warm):                                 # warm-up (buffers, first-launch attributes, clocks)
        fn()
    ctx.prof_reset(); ctx.prof_enable(True)
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        walls.append((time.perf_counter() - t0) * 1e3)
    ctx.prof_enable(False)
    p = ctx.prof_get()["gemm"]
    return p["total_ms"] / reps, float(np.median(walls)), float(min(walls)), p["launches"] / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--users", type=int, default=1000)
    ap.add_argument("--pos", type=int, default=20)
    ap.add_argument("--excl", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--big", type=int, default=100_000)
    ap.add_argument("--only", default="abc")
    args = ap.parse_args()
    from openrec_amd import runtime as rt
    ctx = rt.default_context()
    NU, NI, D = 200_000, args.items, args.dim
    U = rt.Table(NU, D, ctx).init_uniform(seed=0); V = rt.Table(NI, D, ctx).init_uniform(seed=1)
    b = rt.Table(NI, 1, ctx).init_uniform(seed=2); w = rt.Table(D, 1, ctx).init_uniform(seed=3)
    rng = np.random.default_rng(0)

    def lists(n):
        draw = rng.integers(0, NI, (n, args.pos + args.excl))
        return (rt.SparseMask.from_lists([r[:args.pos] for r in draw], NI),
                rt.SparseMask.from_lists([r[args.pos:] for r in draw], NI))
    at = [10, 100]
    uid = rng.integers(0, NU, args.users).astype(np.int32)
    pos, excl = lists(uid.size)
    for kind in ("dot", "gmf", "l2"):
        ww = w if kind == "gmf" else None
        res = {}
        if "a" in args.only:
            ms, wall, wmin, launches, res["a"] = timed(ctx, lambda: rt.rank_metrics_matrixfree(pos, excl, at, kind, U, V, b, uid, w=ww), args.reps)
            nbytes, per = rt.rank_metrics_matrixfree_scratch(uid.size, NI, D, kind, args.pos, args.excl)
            line("a", kind, uid.size, NI, D, ms, wall, {"route": "rank_metrics_matrixfree", "wall_min_ms": wmin, "gemm_launches": launches,
                                                       "scratch_bytes": nbytes, "users_per_batch": per})
        if "b" in args.only:
            ms, wall, wmin, launches, res["b"] = timed(ctx, lambda: rt.rank_metrics_csr(pos, excl, at, kind=kind, user=U, item=V, bias=b, w=ww, uid=uid), args.reps)
            line("b", kind, uid.size, NI, D, ms, wall, {"route": "rank_metrics_csr (score matrix)", "wall_min_ms": wmin, "gemm_launches": launches,
                                                       "score_matrix_bytes": uid.size * NI * 4})
        if len(res) == 2:
            same = all(np.array_equal(res["a"][k], res["b"][k], equal_nan=True) for k in ("auc", "ndcg", "recall"))
            print(json.dumps({"part": "a==b", "kind": kind, "bit_identical": bool(same)}), flush=True)
    if "c" in args.only:
        big = (np.arange(args.big, dtype=np.int64) % NU).astype(np.int32)
        bpos, bexcl = lists(big.size)
        ms, wall, wmin, launches, out = timed(ctx, lambda: rt.rank_metrics_matrixfree(bpos, bexcl, at, "dot", U, V, b, big), 1, warm=0)
        nbytes, per = rt.rank_metrics_matrixfree_scratch(big.size, NI, D, "dot", args.pos, args.excl)
        line("c", "dot", big.size, NI, D, ms, wall, {"route": "rank_metrics_matrixfree", "gemm_launches": launches, "scratch_bytes": nbytes,
                                                    "users_per_batch": per, "score_matrix_gb_avoided": big.size * NI * 4 / 1e9,
                                                    "mean_auc": float(np.nanmean(out["auc"]))})


if __name__ == "__main__":
    main()
