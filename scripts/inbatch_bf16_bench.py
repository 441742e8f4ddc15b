#!/usr/bin/env python3
"""The in-batch step in fp32 and with bf16 operands (`rt.inbatch_step(..., precision="bf16")`) on 1M x 1M tables, D = 64 and 128,
B in {4096, 8192, 16384}, K = 20 per call, SGD with the item bias, ids resident in HBM, no loss read-back -- the protocol of
scripts/inbatch_bench.py and scripts/fullsoftmax_bf16_bench.py: one process, the two forms interleaved call by call on tables of
their own, a host clock around synchronised calls, per form the median time per step over the timed calls and their spread
(max - min).  After the timed calls one profiled K-step call and K profiled forwards per form give the kernels' own times
(orx_prof_*): the three walks sit in the "gemm" slot (the LSE walk alone is read from the forwards), gather / finalize / finish in
"fused".  The fraction of the matrix peak is the walks' 5 * 2 * B^2 * Dp flop against 157 TF (fp32) or 2.5 PF (bf16, dense).  The
gate: the bf16 step is not slower than the fp32 step beyond the two spreads, at every B and D.  Not measured: Adam / Adagrad /
momentum, the step without the bias table, other dims.  The measuring process runs as a child under a time limit of its own.

    python scripts/inbatch_bf16_bench.py [--calls 7] [--warmup 3] [--out profiles/inbatch_bf16_bench.json]
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
K = 20
BS = (4096, 8192, 16384)
PEAK = {"fp32": 157e12, "bf16": 2.5e15}         # MFMA, MI355X, dense


def measure(calls, warmup, batches, dims):
    import torch
    from openrec_amd import runtime as rt
    torch.manual_seed(0)
    ctx = rt.default_context()
    dev = torch.device("cuda", ctx.device)
    out = {"workload": "%dx%d K=%d SGD with the item bias, ids on the device, no read-back" % (NU, NI, K), "calls": calls,
           "warmup": warmup, "peak_flops": PEAK, "not_measured": "Adam / Adagrad / momentum, the step without the bias table, other dims"}
    for D in dims:
        forms = [dict(name=p, o=rt.Optimizer.sgd(0.05),
                      tables=(rt.Table(NU, D).init_uniform(seed=1), rt.Table(NI, D).init_uniform(seed=2), rt.Table(NI, 1).init_uniform(seed=3)))
                 for p in ("fp32", "bf16")]
        for B in batches:
            def ids():
                return (torch.randint(0, NU, (K, B), dtype=torch.int32, device=dev), torch.randint(0, NI, (K, B), dtype=torch.int32, device=dev))

            def call(f):
                uid, pid = ids()
                torch.cuda.synchronize(); ctx.synchronize()
                t0 = time.perf_counter()
                rt.inbatch_step(f["o"], *f["tables"], uid, pid, K=K, B=B, want_loss=False, precision=f["name"])
                ctx.synchronize()
                return (time.perf_counter() - t0) / K * 1e6

            us = {f["name"]: [] for f in forms}
            for it in range(warmup + calls):        # interleaved: both forms see the same machine at the same time
                for f in forms:
                    dt = call(f)
                    if it >= warmup:
                        us[f["name"]].append(dt)
            geo = rt.inbatch_geometry(B, D)
            flop = 5 * 2 * B * B * geo["dim"]
            res = {"geometry": geo, "flop_per_step": flop}
            ctx.prof_enable(True)
            for f in forms:
                uid, pid = ids()
                ctx.prof_reset()
                rt.inbatch_step(f["o"], *f["tables"], uid, pid, K=K, B=B, want_loss=False, precision=f["name"])
                ctx.synchronize()
                st = ctx.prof_get()
                ctx.prof_reset()
                for s in range(K):
                    rt.inbatch_loss(*f["tables"], uid[s], pid[s], precision=f["name"])
                fw = ctx.prof_get()
                lse_us, walks_us, t = fw["gemm"]["total_ms"] / K * 1e3, st["gemm"]["total_ms"] / K * 1e3, us[f["name"]]
                res[f["name"]] = {"us_per_step_median": statistics.median(t), "us_per_step_spread": max(t) - min(t),
                                  "us_per_step": [round(x, 2) for x in t],
                                  "kernels_us_per_step": {
                                      "lse_walk": lse_us, "gradient_walks_both_sides": walks_us - lse_us,
                                      "gather_finalize_finish": st["fused"]["total_ms"] / K * 1e3,
                                      "other_slots": {k: v["total_ms"] / K * 1e3 for k, v in st.items() if k not in ("gemm", "fused") and v["launches"]}},
                                  "fraction_of_peak_walks": flop / (walks_us * 1e-6) / PEAK[f["name"]],
                                  "fraction_of_peak_step": flop / (statistics.median(t) * 1e-6) / PEAK[f["name"]]}
            ctx.prof_enable(False)
            a, b = res["fp32"], res["bf16"]
            res["speedup_bf16"] = a["us_per_step_median"] / b["us_per_step_median"]
            res["gate_bf16_not_slower"] = b["us_per_step_median"] <= a["us_per_step_median"] + a["us_per_step_spread"] + b["us_per_step_spread"]
            out["D%d_B%d" % (D, B)] = res
        del forms
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="*", default=list(BS))
    ap.add_argument("--dims", type=int, nargs="*", default=[64, 128])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inbatch_bf16_bench.json"))
    ap.add_argument("--limit", type=int, default=400, help="seconds the measuring process may take")
    ap.add_argument("--measure", action="store_true", help="(the child) measure in this process and print one JSON line")
    a = ap.parse_args()
    if a.measure:
        print(json.dumps(measure(a.calls, a.warmup, a.batches, a.dims)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--measure", "--calls", str(a.calls),
           "--warmup", str(a.warmup), "--batches"] + [str(n) for n in a.batches] + ["--dims"] + [str(d) for d in a.dims]
    r = subprocess.run(cmd, capture_output=True, text=True)
    sys.stderr.write(r.stderr[-2000:])
    if r.returncode != 0:
        print("the measuring process failed with status %d" % r.returncode)
        return r.returncode
    doc = {"inbatch_bf16": json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])}
    print(json.dumps(doc["inbatch_bf16"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:            # one line per (D, B)
        fh.write('{"inbatch_bf16": {\n' + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in doc["inbatch_bf16"].items()) + "\n}}\n")
    return 0 if all(v["gate_bf16_not_slower"] for k, v in doc["inbatch_bf16"].items() if k.startswith("D")) else 1


if __name__ == "__main__":
    sys.exit(main())
