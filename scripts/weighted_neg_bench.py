#!/usr/bin/env python3
"""Negatives from a weighted item proposal at training scale: `DeviceSampler.pairwise` and `DeviceSampler.pairwise_hard` with 8
candidates on 1 M users x 1 M items x dim 64, n = 65 536 samples per call, each with uniform negatives and with the proposal
count^0.75 over Zipf(1.05) item counts (`set_proposal(popularity=0.75)` on records whose items follow that law).  The uniform
calls of the same run are the yardstick: per call the time (host clock around a batch of back-to-back calls that ends in a
synchronise, divided by the calls; the median over the batches after a warm-up) and, for the weighted ones, the ratio to the
uniform call.  Beside them the share of samples whose negative needed more than one attempt, counted on the host from the
NumPy restatement of the first attempt over one window (uniform and weighted), and the bytes of the alias table.  One JSON line
per measurement, all of them again in `--out`.
    python scripts/weighted_neg_bench.py [--users 1000000] [--items 1000000] [--dim 64] [--n 65536] [--records 4000000] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

U64 = np.uint64


def mix64(x):
    x = np.asarray(x, U64)
    with np.errstate(over="ignore"):
        x = x + U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
        return x ^ (x >> U64(31))


def retry_share(raw, NI, seed, first, uid, table):
    """the share of samples [first, first + len(uid)) whose FIRST attempt is a positive of the user (uid: what the sampler wrote)"""
    keys = np.unique(raw["user_id"].astype(np.int64) * NI + raw["item_id"])
    g = np.arange(first, first + len(uid)).astype(U64)
    with np.errstate(over="ignore"):
        r = mix64(U64(seed) ^ (g * U64(0x9E3779B97F4A7C15)) ^ U64(0xA5A5A5A5))
    item = (r % U64(NI)).astype(np.int64)
    if table is not None:
        thr, alias = table
        t = (mix64(r ^ U64(0x5851F42D4C957F2D)) >> U64(32)).astype(np.uint32)
        item = np.where(t < thr[item], item, alias[item].astype(np.int64))
    k = uid.astype(np.int64) * NI + item
    at = np.minimum(np.searchsorted(keys, k), len(keys) - 1)
    return float((keys[at] == k).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--records", type=int, default=4_000_000)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--zipf", type=float, default=1.05)
    ap.add_argument("--calls", type=int, default=200, help="back-to-back calls per timed batch")
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--model", default="bpr", choices=["bpr", "ucml"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from openrec_amd import runtime as rt
    NU, NI, D, n, M = args.users, args.items, args.dim, args.n, args.candidates
    rng = np.random.default_rng(0)
    law = 1.0 / np.arange(1, NI + 1) ** args.zipf
    cdf = np.cumsum(law); cdf /= cdf[-1]
    rank_to_item = rng.permutation(NI)                       # popularity is not sorted by id
    raw = np.zeros(args.records, dtype=[("user_id", np.int32), ("item_id", np.int32)])
    raw["user_id"] = rng.integers(0, NU, args.records)
    raw["item_id"] = rank_to_item[np.minimum(np.searchsorted(cdf, rng.random(args.records)), NI - 1)]
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

    shape = {"users": NU, "items": NI, "dim": D, "n": n, "records": args.records, "model": args.model, "zipf": args.zipf,
             "alpha": args.alpha, "calls_per_batch": args.calls, "batches": args.batches}
    calls = {"pairwise": lambda k: sm.pairwise(5, k * n, n, uid, pid, nid),
             "pairwise_hard": lambda k: sm.pairwise_hard(5, k * n, n, uid, pid, nid, args.model, U, V, b, candidates=M)}
    res = {}
    for proposal in ("uniform", "weighted", "uniform", "weighted"):      # alternating: two rounds of each, the better median counts
        sm.set_proposal(None) if proposal == "uniform" else sm.set_proposal(popularity=args.alpha)
        table = sm.proposal()
        sm.pairwise(5, 0, n, uid, pid, nid); ctx.synchronize()
        share = retry_share(raw, NI, 5, 0, uid.cpu().numpy(), table)
        for name, fn in calls.items():
            med, lo = timed(fn)
            key = (name, proposal)
            if key not in res or med < res[key]["ms_median"]:
                res[key] = {"part": name, "call": "DeviceSampler." + name, "proposal": proposal,
                            "candidates": M if name == "pairwise_hard" else 1, **shape, "ms_median": med, "ms_min": lo,
                            "share_of_samples_with_more_than_one_attempt": share,
                            "table_bytes": 0 if table is None else 8 * NI}
    for name in calls:
        u, w = res[(name, "uniform")], res[(name, "weighted")]
        w["ratio_to_uniform"] = w["ms_median"] / u["ms_median"]
        w["extra_us"] = (w["ms_median"] - u["ms_median"]) * 1e3
        emit(u); emit(w)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
