#!/usr/bin/env python3
"""Evaluation against sampled negatives at evaluation scale: `model.evaluate` on 1 000 users x 1 M items x dim 64 with 1 000
candidates per user (20 positives among them), through `cand_mask` (orx_rank_metrics_candidates: only the listed items are
scored) and through the only other route for this protocol, the dense `excl_mask` = everything but the candidates with the
default `score_matrix`.  Each timed repetition includes the host work of building the masks in the form `Dataset.evaluation`
hands them out and shipping them; the median of the repetitions after a warm-up is reported.  Also: the candidate scorer's
kernel time (dispatch-attached events, `score_candidates(device=True)`) against its byte model -- 4 D bytes per entry for the
row, 4 for the id, 4 for the bias, 4 written -- at the copy rate `orx_copy_bandwidth` measures in the same process.
One JSON line per measurement, all of them again in `--out`.
    python scripts/cand_eval_bench.py [--items 1000000] [--users 1000] [--dim 64] [--cand 1000] [--pos 20] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--users", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--cand", type=int, default=1000)
    ap.add_argument("--pos", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dense-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from openrec_amd import runtime as rt
    from openrec_amd.tf2.recommenders import BPR
    NU, NI, D, n = 200_000, args.items, args.dim, args.users
    m = BPR(D, D, NU, NI)
    U, V, b = m._tables()
    ctx = U.ctx
    U.init_uniform(seed=0); V.init_uniform(seed=1); b.init_uniform(seed=2)
    rng = np.random.default_rng(0)
    uid = rng.integers(0, NU, n).astype(np.int32)
    cand_rows = [np.unique(rng.integers(0, NI, args.cand)) for _ in range(n)]
    pos_rows = [rng.choice(r, args.pos, replace=False) for r in cand_rows]
    at = [10, 100]
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    def via_cand():
        pos, cand = rt.SparseMask.from_lists(pos_rows, NI), rt.SparseMask.from_lists(cand_rows, NI)
        return m.evaluate(uid, pos, at=at, cand_mask=cand)

    def via_dense():
        pos = rt.SparseMask.from_lists(pos_rows, NI)
        excl = np.ones((n, NI), bool)                      # what Dataset.evaluation builds with explicit negatives
        for q, r in enumerate(cand_rows):
            excl[q, r] = False
        return m.evaluate(uid, pos, excl, at=at)

    def timed(fn, reps, warm=1):
        for _ in range(warm):
            out = fn()
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            walls.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(walls)), float(min(walls)), out

    shape = {"users": n, "items": NI, "dim": D, "candidates_per_user": float(np.mean([len(r) for r in cand_rows])), "positives": args.pos}
    wall_c, min_c, out_c = timed(via_cand, args.reps, warm=2)
    emit({"part": "evaluate", "route": "cand_mask (rank_metrics_candidates)", **shape, "wall_ms_median": wall_c, "wall_ms_min": min_c,
          "reps": args.reps, "mask_bytes_shipped": int(sum(map(len, cand_rows)) + sum(map(len, pos_rows))) * 4})
    wall_d, min_d, out_d = timed(via_dense, args.dense_reps, warm=1)
    emit({"part": "evaluate", "route": "dense excl_mask, score_matrix=True (rank_metrics)", **shape, "wall_ms_median": wall_d,
          "wall_ms_min": min_d, "reps": args.dense_reps, "mask_bytes_shipped": 2 * n * NI})
    # the dense-mask kernel adds a user's NDCG terms with float atomics in no fixed order: AUC and Recall are equal bit for
    # bit, NDCG to the rounding of a re-ordered sum; the list route (rank_metrics_csr on the complement) is equal throughout
    same = {k: bool(np.array_equal(out_c[k], out_d[k], equal_nan=True)) for k in ("auc", "ndcg", "recall")}
    emit({"part": "evaluate", "equal_to_dense_route": same,
          "ndcg_max_rel_diff": float(np.nanmax(np.abs(out_c["ndcg"] - out_d["ndcg"]) / np.maximum(out_d["ndcg"], 1e-30))),
          "speedup_wall_median": wall_d / wall_c, "mean_auc": float(np.nanmean(out_c["auc"]))})

    # the candidate scorer alone against its byte model at this device's copy rate
    gbps = ctx.copy_bandwidth(1 << 30, 10)
    cand = rt.SparseMask.from_lists(cand_rows, NI)
    entries = int(cand.ptr[-1])
    for _ in range(3):
        rt.score_candidates("dot", U, V, b, uid, cand, device=True)
    ctx.synchronize()
    reps = 10
    per = []
    for _ in range(reps):                                  # one launch per repetition: each one's own kernel time
        ctx.prof_reset(); ctx.prof_enable(True)
        rt.score_candidates("dot", U, V, b, uid, cand, device=True)
        ctx.synchronize(); ctx.prof_enable(False)
        per.append(ctx.prof_get()["gemm"]["total_ms"])
    model_bytes = entries * (4 * D + 12)
    floor_ms = model_bytes / (gbps * 1e9) * 1e3
    emit({"part": "scorer", "kernel": "cand_score_kernel", "entries": entries, "dim": D, "kernel_ms_median": float(np.median(per)),
          "kernel_ms_min": float(min(per)), "reps": reps, "model_bytes": model_bytes, "copy_gbps": gbps, "model_ms_at_copy_rate": floor_ms,
          "frac_of_copy_rate": floor_ms / float(np.median(per))})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
