#!/usr/bin/env python3
"""The conjugate-gradient ALS half-step (`rt.als_half_step(..., solver="cg")`) against the Cholesky one, and `rt.als_objective`,
on the data set of scripts/als_bench.py: 1M users x 1M items, about 20M observations, items ~ Zipf(1.05) and users uniform, and
the variant with the items uniform; D = 64 and 128; the CSRs resident in HBM.

  times        Cholesky and CG at cg_steps = 1, 3 and 5, user half-step and item half-step, INTERLEAVED in one process: round i
               runs every variant once, so drift of the machine falls on all of them alike.  Per figure the median of `--calls`
               synchronised calls after `--warmup`, a host clock around them, with the spread (max - min).  `cg3_speedup` is the
               Cholesky median over the CG-3 median of the same half-step.
  objective    the time of `rt.als_objective` on the same tables (it synchronises by itself)
  convergence  the objective after each of 5 sweeps, for Cholesky and for CG-3 from the same start (Zipf set only): what the inexact
               solve costs in descent

The measuring process runs as a child under a time limit of its own; a failure ends the script.  Results go to `--out`,
profiles/als_cg_bench.json.

    python scripts/als_cg_bench.py [--calls 5] [--warmup 2] [--out profiles/als_cg_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

A, B, REG = 5.0, 1.0, 0.1
VARIANTS = (("cholesky", dict(solver="cholesky")), ("cg1", dict(solver="cg", cg_steps=1)), ("cg3", dict(solver="cg", cg_steps=3)),
            ("cg5", dict(solver="cg", cg_steps=5)))
SWEEPS = 5


def measure(calls, warmup):
    import numpy as np
    import torch
    import als_bench
    from openrec_amd import runtime as rt
    ctx = rt.default_context()

    def clock(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def summary(ts):
        ts = ts[warmup:]
        return dict(ms_median=statistics.median(ts), ms_spread=max(ts) - min(ts), ms=[round(t, 3) for t in ts])

    out = {"workload": "%d x %d, %d records before duplicates merge, confidences a = %g, b = %g, reg = %g, CSRs on the device"
                       % (als_bench.NU, als_bench.NI, als_bench.NNZ, A, B, REG),
           "calls": calls, "warmup": warmup, "row_breaks": {str(D): rt.als_cg_row_breaks(D) for D in (64, 128)}}
    for name, zipf in (("zipf_1.05", True), ("uniform", False)):
        data = rt.ALSData(als_bench.records(zipf), als_bench.NU, als_bench.NI, ctx=ctx)
        lens = np.diff(data.by_item.ptr)
        res = {"nnz": data.nnz, "longest_item_row": int(lens.max()), "mean_user_row": float(np.diff(data.by_user.ptr).mean())}
        for D in (64, 128):
            U = rt.Table(als_bench.NU, D).init_uniform(seed=1); V = rt.Table(als_bench.NI, D).init_uniform(seed=2)
            U0, V0 = U.read(), V.read()
            ts = {v: {"user_half": [], "item_half": []} for v, _ in VARIANTS}
            tobj = []
            for _ in range(warmup + calls):                 # one round: every variant once
                for v, kw in VARIANTS:
                    ts[v]["user_half"].append(clock(lambda: rt.als_half_step(V, U, data.by_user, A, B, REG, **kw)))
                    ts[v]["item_half"].append(clock(lambda: rt.als_half_step(U, V, data.by_item, A, B, REG, **kw)))
                tobj.append(clock(lambda: rt.als_objective(U, V, data, A, B, REG)))
            r = {v: {h: summary(t) for h, t in d.items()} for v, d in ts.items()}
            r["objective"] = summary(tobj)
            r["cg3_speedup"] = {h: r["cholesky"][h]["ms_median"] / r["cg3"][h]["ms_median"] for h in ("user_half", "item_half")}
            if zipf:
                conv = {}
                for v in ("cholesky", "cg3"):
                    kw = dict(VARIANTS)[v]
                    U.write(U0); V.write(V0)
                    obj = [rt.als_objective(U, V, data, A, B, REG)]
                    for _ in range(SWEEPS):
                        rt.als_sweep(U, V, data, A, B, REG, **kw)
                        obj.append(rt.als_objective(U, V, data, A, B, REG))
                    conv[v] = obj
                r["objective_after_sweeps"] = conv
            res["D%d" % D] = r
            print(name, D, json.dumps({v: {h: round(r[v][h]["ms_median"], 3) for h in ("user_half", "item_half")} for v, _ in VARIANTS}),
                  "objective ms", round(r["objective"]["ms_median"], 3), file=sys.stderr, flush=True)
            del U, V
        out[name] = res
        del data
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_cg_bench.json"))
    ap.add_argument("--limit", type=int, default=840, help="seconds the measuring process may take")
    ap.add_argument("--measure", action="store_true", help="(the child) measure in this process and print one JSON line")
    a = ap.parse_args()
    if a.measure:
        print(json.dumps(measure(a.calls, a.warmup)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--measure", "--calls", str(a.calls), "--warmup", str(a.warmup)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        print("the measuring process failed with status %d" % r.returncode)
        return r.returncode
    doc = {"als_cg_bench": json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])}
    print(json.dumps(doc["als_cg_bench"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
