#!/usr/bin/env python3
"""The time of the in-batch step (`rt.inbatch_step`) at 1M x 1M x 64, B in {4096, 8192, 16384}, K = 20 per call, SGD with the
item bias, ids resident in HBM, no loss read-back, and -- for context only -- `rt.multineg_step("softmax", N = 64)` at the same B,
which is a DIFFERENT objective (64 drawn negatives per positive against B - 1 in-batch ones) and therefore a yardstick, not a bar.
One process, the forms interleaved call by call on tables of their own, a host clock around synchronised calls; per form the
median time per step over the timed calls and their spread (max - min).  After the timed calls, one profiled call per B gives the
kernels' own times from the dispatch-attached events (orx_prof_*): the three MFMA walks sit in the "gemm" slot (the LSE walk alone
is read from a profiled `rt.inbatch_loss`), gather / finalize / finish in "fused"; and the achieved fraction of the 157 TF fp32
matrix peak on the count 5 * 2 * B^2 * Dp.  Not measured here: other dims, Adam / Adagrad / momentum, the step without the bias.
The measuring process runs as a child under a time limit of its own; a failure ends the script.  Results go to `--out`,
profiles/inbatch_bench.json.

    python scripts/inbatch_bench.py [--calls 7] [--warmup 3] [--out profiles/inbatch_bench.json]
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

NU = NI = 1_000_000
D, K = 64, 20
BS = (4096, 8192, 16384)
PEAK = 157e12                                 # fp32 MFMA, MI355X


def measure(calls, warmup):
    import torch
    from openrec_amd import runtime as rt
    torch.manual_seed(0)
    ctx = rt.default_context()
    forms = []
    for B in BS:
        for kind in ("inbatch", "multineg_softmax_N64"):
            tU = rt.Table(NU, D).init_uniform(seed=1); tV = rt.Table(NI, D).init_uniform(seed=2); tb = rt.Table(NI, 1).init_uniform(seed=3)
            forms.append(dict(name=f"{kind}_B{B}", kind=kind, B=B, tables=(tU, tV, tb), o=rt.Optimizer.sgd(0.05), us=[]))

    def ids(B, steps):
        return (torch.randint(0, NU, (steps, B), dtype=torch.int32, device="cuda"),
                torch.randint(0, NI, (steps, B), dtype=torch.int32, device="cuda"))

    def call(f):
        B = f["B"]
        uid, pid = ids(B, K)
        nid = torch.randint(0, NI, (K, B, 64), dtype=torch.int32, device="cuda") if f["kind"] != "inbatch" else None
        torch.cuda.synchronize(); ctx.synchronize()
        t0 = time.perf_counter()
        if nid is None:
            rt.inbatch_step(f["o"], *f["tables"], uid, pid, K=K, B=B, want_loss=False)
        else:
            rt.multineg_step("softmax", f["o"], *f["tables"], uid, pid, nid, K=K, B=B, want_loss=False)
        ctx.synchronize()
        return (time.perf_counter() - t0) / K * 1e6

    for it in range(warmup + calls):            # interleaved: every form sees the same box at the same time
        for f in forms:
            dt = call(f)
            if it >= warmup:
                f["us"].append(dt)
    out = {"workload": "D=%d %dx%d K=%d SGD with the item bias, ids on the device, no read-back" % (D, NU, NI, K),
           "calls": calls, "warmup": warmup, "peak_flops": PEAK,
           "note": "multineg_softmax_N64: a different objective (64 drawn negatives), quoted as a yardstick only",
           "not_measured": "other dims, Adam / Adagrad / momentum, the step without the bias table"}
    for f in forms:
        out[f["name"]] = {"us_per_step_median": statistics.median(f["us"]), "us_per_step_spread": max(f["us"]) - min(f["us"]),
                          "us_per_step": [round(t, 2) for t in f["us"]]}
    # the kernels' own times: one profiled K-step call and K profiled forwards per B
    ctx.prof_enable(True)
    for f in (f for f in forms if f["kind"] == "inbatch"):
        B = f["B"]
        geo = rt.inbatch_geometry(B, D)
        uid, pid = ids(B, K)
        ctx.prof_reset()
        rt.inbatch_step(f["o"], *f["tables"], uid, pid, K=K, B=B, want_loss=False)
        ctx.synchronize()
        step = ctx.prof_get()
        ctx.prof_reset()
        for s in range(K):
            rt.inbatch_loss(*f["tables"], uid[s], pid[s])
        fwd = ctx.prof_get()
        lse_us = fwd["gemm"]["total_ms"] / K * 1e3
        walks_us = step["gemm"]["total_ms"] / K * 1e3
        flop = 5 * 2 * B * B * geo["dim"]
        out[f["name"]]["geometry"] = geo
        out[f["name"]]["kernels_us_per_step"] = {
            "lse_walk": lse_us, "gradient_walks_both_sides": walks_us - lse_us,
            "gather_finalize_finish": step["fused"]["total_ms"] / K * 1e3,
            "other_slots": {k: v["total_ms"] / K * 1e3 for k, v in step.items() if k not in ("gemm", "fused") and v["launches"]}}
        out[f["name"]]["flop_per_step"] = flop
        out[f["name"]]["fraction_of_peak_walks"] = flop / (walks_us * 1e-6) / PEAK
        out[f["name"]]["fraction_of_peak_step"] = flop / (out[f["name"]]["us_per_step_median"] * 1e-6) / PEAK
    ctx.prof_enable(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inbatch_bench.json"))
    ap.add_argument("--limit", type=int, default=400, help="seconds the measuring process may take")
    ap.add_argument("--measure", action="store_true", help="(the child) measure in this process and print one JSON line")
    a = ap.parse_args()
    if a.measure:
        print(json.dumps(measure(a.calls, a.warmup)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--measure", "--calls", str(a.calls), "--warmup", str(a.warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    sys.stderr.write(r.stderr[-2000:])
    if r.returncode != 0:
        print("the measuring process failed with status %d" % r.returncode)
        return r.returncode
    doc = {"inbatch_step": json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])}
    print(json.dumps(doc["inbatch_step"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
