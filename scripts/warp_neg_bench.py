#!/usr/bin/env python3
"""WARP negative sampling at training scale: `DeviceSampler.pairwise_warp` on 1 M users x 1 M items x dim 64, n = 65 536 samples
per call, T = 16, ids and tables resident, 4 M records.  Three regimes set by the margin alone on the random tables:
(a) +inf, every sample violates at once; (b) 0, the natural mix; (c) -inf, nothing violates.  Alternating with each regime, in the
same process, `DeviceSampler.pairwise_hard` at M = 16: the fixed-M call that pays the worst case for every sample.  Timing as
scripts/hard_neg_bench.py: the host clock around a batch of back-to-back calls that ends in a synchronise, divided by the calls,
the median over the batches after a warm-up; the float4 copy rate `orx_copy_bandwidth` in the same process.  Per regime: the time
of a call, the mean number of candidates the contract has scored per sample (t, or T when t = 0, from `trials_out`), the byte model
n (E[candidates] + 2)(4 D + 4) -- the candidates' rows, the positive's and the user's -- and that traffic as a fraction of the
copy rate.  One JSON line per measurement, all of them again in `--out`.

    python scripts/warp_neg_bench.py [--users 1000000] [--items 1000000] [--dim 64] [--n 65536] [--trials 16] [--out FILE]

`--hard-runs DIR` (no device needed) adds to `--out` the medians of scripts/hard_neg_bench.py outputs DIR/hard_parent_*.json and
DIR/hard_this_*.json: the no-regression comparison of `pairwise_hard` between the parent's build and this one."""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def merge_hard_runs(directory, out):
    res = {"part": "pairwise_hard_parent_vs_this", "script": "scripts/hard_neg_bench.py"}
    for side in ("parent", "this"):
        runs = [json.load(open(f)) for f in sorted(glob.glob(os.path.join(directory, f"hard_{side}_*.json")))]
        per = {}
        for run in runs:
            for d in run:
                if d["part"] in ("draw", "hard"):
                    per.setdefault("pairwise" if d["part"] == "draw" else f"M={d['candidates']}", []).append(d["ms_median"] * 1e3)
        res[side] = {k: {"us_per_run": v, "us_median": float(np.median(v)), "us_spread": float(max(v) - min(v))} for k, v in per.items()}
        res[side + "_runs"] = len(runs)
    lines = json.load(open(out)) if os.path.exists(out) else []
    lines = [d for d in lines if d.get("part") != res["part"]] + [res]
    with open(out, "w") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--records", type=int, default=4_000_000)
    ap.add_argument("--trials", type=int, default=16)
    ap.add_argument("--calls", type=int, default=200, help="back-to-back calls per timed batch")
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--model", default="bpr", choices=["bpr", "ucml"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--hard-runs", default=None)
    args = ap.parse_args()
    if args.hard_runs:
        return merge_hard_runs(args.hard_runs, args.out)
    import torch
    from openrec_amd import runtime as rt
    NU, NI, D, n, T = args.users, args.items, args.dim, args.n, args.trials
    rng = np.random.default_rng(0)
    raw = np.zeros(args.records, dtype=[("user_id", np.int32), ("item_id", np.int32)])
    raw["user_id"] = rng.integers(0, NU, args.records); raw["item_id"] = rng.integers(0, NI, args.records)
    ctx = rt.default_context()
    sm = rt.DeviceSampler(raw, NU, NI, ctx)
    U = rt.Table(NU, D).init_uniform(seed=0); V = rt.Table(NI, D).init_uniform(seed=1); b = rt.Table(NI, 1).init_uniform(seed=2)
    dev = torch.device("cuda", 0)
    uid, pid, nid, trials = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
    w = torch.empty(n, dtype=torch.float32, device=dev)
    table = rt.warp_weights(NI, T, "log")
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
    shape = {"users": NU, "items": NI, "dim": D, "n": n, "records": args.records, "model": args.model, "max_trials": T,
             "calls_per_batch": args.calls, "batches": args.batches, "copy_gbps": gbps,
             "chunk_env": os.environ.get("ORX_WARP_CHUNK"), "slots_env": os.environ.get("ORX_WARP_SLOTS")}
    hard_bytes = n * (T + 1) * (4 * D + 4)
    for regime, margin in (("a: every sample violates at once", np.inf), ("b: the natural mix", 0.0), ("c: nothing violates", -np.inf)):
        hard_med, hard_lo = timed(lambda k: sm.pairwise_hard(5, k * n, n, uid, pid, nid, args.model, U, V, b, candidates=T))
        med, lo = timed(lambda k: sm.pairwise_warp(5, k * n, n, uid, pid, nid, w, args.model, U, V, b, max_trials=T, margin=margin,
                                                   rank_weight=table))
        # the trial counts of 16 windows of the stream
        scored, none, first = [], [], []
        for k in range(16):
            sm.pairwise_warp(5, k * n, n, uid, pid, nid, w, args.model, U, V, b, max_trials=T, margin=margin, rank_weight=table,
                             trials_out=trials)
            ctx.synchronize()
            t = trials.cpu().numpy()
            scored.append(np.where(t > 0, t, T).mean()); none.append((t == 0).mean()); first.append(t[t > 0].mean() if (t > 0).any() else 0.0)
        e = float(np.mean(scored))
        model_bytes = n * (e + 2) * (4 * D + 4)
        floor_ms = model_bytes / (gbps * 1e9) * 1e3
        emit({"part": "warp", "call": "DeviceSampler.pairwise_warp", "regime": regime, "margin": str(margin), **shape,
              "ms_median": med, "ms_min": lo, "mean_candidates_scored": e, "share_without_violator": float(np.mean(none)),
              "mean_trials_of_the_violated": float(np.mean(first)), "model_bytes": model_bytes, "model_ms_at_copy_rate": floor_ms,
              "frac_of_copy_rate": floor_ms / med,
              "pairwise_hard_M16_ms_median": hard_med, "pairwise_hard_M16_ms_min": hard_lo, "pairwise_hard_M16_model_bytes": hard_bytes,
              "ratio_to_pairwise_hard_M16": med / hard_med, "byte_model_ratio_to_pairwise_hard_M16": model_bytes / hard_bytes})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
