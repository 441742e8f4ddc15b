#!/usr/bin/env python3
"""The full-softmax step in fp32 and with bf16 operands (`rt.fullsoftmax_step(..., precision="bf16")`) at B = 4096 over
25 000 / 100 000 / 1 000 000 items, D = 64 and once more D = 128, under SGD, ids resident in HBM, no loss read-back -- the
protocol of scripts/fullsoftmax_bench.py: one process, the two forms interleaved call by call on tables of their own, a host
clock around synchronised calls, per form the median over the timed calls and their spread (max - min).  After the timed calls
one profiled step and one profiled forward per form give the kernels' own times (orx_prof_*): the walks sit in the "gemm" slot
(the LSE walk alone is read from the forward), prepare / item copy / bf16 copies / finalize / finish in "fused".  The fraction
of the matrix peak is the walks' 5 * 2 * B * NIp * Dp flop against 157 TF (fp32) or 2.5 PF (bf16, dense).  The gate: the bf16
step is not slower than the fp32 step beyond the two spreads, at every item count.  The measuring process runs as a child under a
time limit of its own.

    python scripts/fullsoftmax_bf16_bench.py [--calls 7] [--warmup 3] [--out profiles/fullsoftmax_bf16_bench.json]
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

B, NU = 4096, 100_000
ITEMS = (25_000, 100_000, 1_000_000)
PEAK = {"fp32": 157e12, "bf16": 2.5e15}         # MFMA, MI355X, dense


def measure(calls, warmup, items, dims):
    import torch
    from openrec_amd import runtime as rt
    torch.manual_seed(0)
    ctx = rt.default_context()
    dev = torch.device("cuda", ctx.device)
    out = {"workload": "B=%d, user-table form, SGD, ids on the device, no read-back" % B, "calls": calls, "warmup": warmup,
           "peak_flops": PEAK, "not_measured": "other B, Adam / Adagrad / momentum, the SeqRec and tower forms, weights and offsets"}
    for D in dims:
        for NI in items:
            forms = [dict(name=p, us=[], o=rt.Optimizer.sgd(0.05),
                          tables=(rt.Table(NU, D).init_uniform(seed=1), rt.Table(NI, D).init_uniform(seed=2), rt.Table(NI, 1).init_uniform(seed=3)))
                     for p in ("fp32", "bf16")]

            def step(f, forward=False):
                uid = torch.randint(0, NU, (B,), dtype=torch.int32, device=dev)
                pid = torch.randint(0, NI, (B,), dtype=torch.int32, device=dev)
                torch.cuda.synchronize(); ctx.synchronize()
                t0 = time.perf_counter()
                if forward:
                    rt.fullsoftmax_loss(*f["tables"], uid, pid, precision=f["name"])
                else:
                    rt.fullsoftmax_step(f["o"], *f["tables"], uid, pid, want_loss=False, precision=f["name"])
                ctx.synchronize()
                return (time.perf_counter() - t0) * 1e6

            for it in range(warmup + calls):        # interleaved: both forms see the same machine at the same time
                for f in forms:
                    dt = step(f)
                    if it >= warmup:
                        f["us"].append(dt)
            geo = rt.fullsoftmax_geometry(B, NI, D)
            flop = 5 * 2 * B * (-(-NI // 64) * 64) * geo["dim"]
            res = {"geometry": geo, "flop_per_step": flop}
            ctx.prof_enable(True)
            for f in forms:
                ctx.prof_reset(); step(f); st = ctx.prof_get()
                ctx.prof_reset(); step(f, forward=True); fw = ctx.prof_get()
                lse_us, walks_us = fw["gemm"]["total_ms"] * 1e3, st["gemm"]["total_ms"] * 1e3
                res[f["name"]] = {"us_per_step_median": statistics.median(f["us"]), "us_per_step_spread": max(f["us"]) - min(f["us"]),
                                  "us_per_step": [round(t, 2) for t in f["us"]],
                                  "kernels_us_per_step": {"lse_walk": lse_us, "gradient_walks_both_sides": walks_us - lse_us,
                                                          "fused_slot": st["fused"]["total_ms"] * 1e3},
                                  "fraction_of_peak_lse_walk": flop / 5 / (lse_us * 1e-6) / PEAK[f["name"]],
                                  "fraction_of_peak_gradient_walks": flop * 4 / 5 / ((walks_us - lse_us) * 1e-6) / PEAK[f["name"]]}
            ctx.prof_enable(False)
            a, b = res["fp32"], res["bf16"]
            res["speedup_bf16"] = a["us_per_step_median"] / b["us_per_step_median"]
            res["gate_bf16_not_slower"] = b["us_per_step_median"] <= a["us_per_step_median"] + a["us_per_step_spread"] + b["us_per_step_spread"]
            out["D%d_items_%d" % (D, NI)] = res
            del forms
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--items", type=int, nargs="*", default=list(ITEMS))
    ap.add_argument("--dims", type=int, nargs="*", default=[64, 128])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fullsoftmax_bf16_bench.json"))
    ap.add_argument("--limit", type=int, default=400, help="seconds the measuring process may take")
    ap.add_argument("--measure", action="store_true", help="(the child) measure in this process and print one JSON line")
    a = ap.parse_args()
    if a.measure:
        print(json.dumps(measure(a.calls, a.warmup, a.items, a.dims)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--measure", "--calls", str(a.calls),
           "--warmup", str(a.warmup), "--items"] + [str(n) for n in a.items] + ["--dims"] + [str(d) for d in a.dims]
    r = subprocess.run(cmd, capture_output=True, text=True)
    sys.stderr.write(r.stderr[-2000:])
    if r.returncode != 0:
        print("the measuring process failed with status %d" % r.returncode)
        return r.returncode
    doc = {"fullsoftmax_bf16": json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])}
    print(json.dumps(doc["fullsoftmax_bf16"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0 if all(v["gate_bf16_not_slower"] for k, v in doc["fullsoftmax_bf16"].items() if k.startswith("D")) else 1


if __name__ == "__main__":
    sys.exit(main())
