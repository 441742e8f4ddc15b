#!/usr/bin/env python3
"""recommend_topk with and without the bf16 prefilter (ORX_TOPK_BF16_PREFILTER), interleaved in one process on the same tables:
1 000 users x 1 M items x dim 64, k in {10, 100, 1000}, dot / GMF / L2 with 200 excluded items per user, and 100 000 users at
k = 100 (dot).  The yardstick is the route the call takes without the flag.  Kernel time from the dispatch-attached events of
the ORX_K_GEMM slot; the split of a prefiltered call comes from ORX_PROF_TIMELINE's per-launch durations, read in launch order
(item copy | per batch: threshold scorer + threshold select, filter, re-score, select); it is left out when a dense fallback
added launches.  The outputs of the two routes are compared bit for bit.  Writes profiles/topk_bf16_bench.json.
    python scripts/topk_bf16_bench.py [--items 1000000] [--dim 64] [--excl 200] [--reps 3] [--big 100000] [--out FILE]"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["ORX_PROF_TIMELINE"] = "1"


class Stderr:
    """file descriptor 2 into a temporary file for the length of a `with`: the library prints its timeline there"""
    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2); os.close(self.saved)
        self.tmp.seek(0); self.text = self.tmp.read(); self.tmp.close()


def timed(ctx, fn, reps):
    """-> (kernel ms per call, wall ms per call, launches per call, per-launch durations in us of all reps, the last result)"""
    ctx.prof_reset(); ctx.prof_enable(True)
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    wall = (time.perf_counter() - t0) / reps * 1e3
    ctx.prof_enable(False)
    with Stderr() as err:
        p = ctx.prof_get()["gemm"]
    durs = [float(m.group(1)) for m in re.finditer(r"gap\s+([0-9.]+) us\s+class", err.text)]
    return p["total_ms"] / reps, wall, p["launches"] // reps, durs, out


def split(durs, reps, launches, batches):
    """the phases of a prefiltered call from its launches, in ms per call"""
    if launches != 1 + 5 * batches or len(durs) != reps * launches:
        return None
    s = dict(item_copy=0.0, threshold=0.0, filter=0.0, rescore=0.0, select=0.0)
    for r in range(reps):
        d = durs[r * launches:(r + 1) * launches]
        s["item_copy"] += d[0]
        for b in range(batches):
            e = d[1 + 5 * b:6 + 5 * b]
            s["threshold"] += e[0] + e[1]; s["filter"] += e[2]; s["rescore"] += e[3]; s["select"] += e[4]
    return {k: v / reps * 1e-3 for k, v in s.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--excl", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--big", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_bf16_bench.json"))
    args = ap.parse_args()
    from openrec_amd import runtime as rt
    ctx = rt.default_context()
    NU, NI, D = 200_000, args.items, args.dim
    U = rt.Table(NU, D, ctx).init_uniform(seed=0); V = rt.Table(NI, D, ctx).init_uniform(seed=1)
    b = rt.Table(NI, 1, ctx).init_uniform(seed=2); w = rt.Table(D, 1, ctx).init_uniform(seed=3)
    rng = np.random.default_rng(0)
    uid = rng.integers(0, NU, 1000).astype(np.int32)
    excl = rt.SparseMask.from_lists([rng.choice(NI, args.excl, replace=False) for _ in range(uid.size)], NI)
    cases = [(kind, k, uid, excl, args.reps) for kind in ("dot", "gmf", "l2") for k in (10, 100, 1000)]
    if args.big:
        cases.append(("dot", 100, np.arange(args.big, dtype=np.int32), None, 1))
    results = []
    for kind, k, ids, ex, reps in cases:
        call = {pf: (lambda pf=pf: rt.recommend_topk(kind, U, V, b, ids, k, excl=ex, w=w, prefilter=pf)) for pf in (None, "bf16")}
        geo = rt.topk_geometry(kind, ids.size, NI, D, k, prefilter="bf16")
        if ids.size <= 1000:
            for pf in call:
                call[pf]()                              # warm-up: buffers, first-launch attributes
        acc = {None: [0.0, 0.0], "bf16": [0.0, 0.0]}
        durs16, launches16 = [], 0
        for _ in range(reps):                           # interleaved: one call of each route, reps times
            for pf in (None, "bf16"):
                ms, wall, launches, durs, out = timed(ctx, call[pf], 1)
                acc[pf][0] += ms / reps; acc[pf][1] += wall / reps
                if pf:
                    durs16 += durs; launches16 = launches
                    stat = {s: ctx.stat(s) for s in ("topk_prefiltered", "topk_dense", "topk_candidates")}
                    got16 = out
                else:
                    got32 = out
        same = bool((got16[0] == got32[0]).all() and (got16[1].view(np.int32) == got32[1].view(np.int32)).all())
        batches = -(-ids.size // geo["batch_users"])
        d = {"kind": kind, "users": int(ids.size), "items": NI, "dim": D, "k": k, "excluded_per_user": args.excl if ex is not None else 0,
             "fp32_route_kernel_ms": acc[None][0], "fp32_route_wall_ms": acc[None][1],
             "fp32_route": rt.topk_geometry(kind, ids.size, NI, D, k)["route"],
             "bf16_prefilter_kernel_ms": acc["bf16"][0], "bf16_prefilter_wall_ms": acc["bf16"][1], "route": geo["route"],
             "speedup_kernel": acc[None][0] / acc["bf16"][0], "split_ms": split(durs16, reps, launches16, batches),
             "candidates_per_user": stat["topk_candidates"] / max(1, stat["topk_prefiltered"]), "topk_dense": stat["topk_dense"],
             "bit_identical": same, "geometry": geo}
        print(json.dumps(d), flush=True)
        results.append(d)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
