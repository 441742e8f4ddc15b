#!/usr/bin/env python3
"""The sampled-softmax step over a shared candidate list in fp32 and with bf16 operands
(`rt.sampled_softmax_step(..., precision="bf16")`) at 1M users x 1M items, B = 4096, S in {1024, 8192}, D = 64 (and 128), SGD
with the item bias, ids resident in HBM, no loss read-back -- the shapes of scripts/sampled_softmax_bench.py, the protocol of
scripts/inbatch_bf16_bench.py: one process, the two forms interleaved call by call on tables of their own, a host clock around
synchronised calls, per form the median over the timed calls and their spread (max - min).  After the timed calls, per form, one
profiled step, one with the user table alone trained (no column kernel) and one profiled forward give the kernels' own times
from the dispatch-attached events (orx_prof_*): the walks sit in the "gemm" slot -- fp32: the fused row kernel and the column
kernel; bf16: the stats walk (read from the forward), the query-gradient walk, the column walk --, gather / merge / finish in
"fused".  The fraction of the matrix peak is on the count 2 B Sp Dk per product, five products a step, against 157 TF (fp32) or
2.5 PF (bf16, dense).  Not measured: other B, Adam / Adagrad / momentum, the SeqRec form, weights and offsets, host id lists.
The measuring process runs as a child under a time limit of its own.

    python scripts/sampled_softmax_bf16_bench.py [--calls 9] [--warmup 3] [--out profiles/sampled_softmax_bf16_bench.json]
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

B, NU, NI = 4096, 1_000_000, 1_000_000
CANDS = (1024, 8192)
PEAK = {"fp32": 157e12, "bf16": 2.5e15}         # MFMA, MI355X, dense


def measure(calls, warmup, cands, dims):
    import torch
    from openrec_amd import runtime as rt
    torch.manual_seed(0)
    ctx = rt.default_context()
    dev = torch.device("cuda", ctx.device)
    out = {"workload": "B=%d, %d users x %d items, SGD with the item bias, ids on the device, no read-back" % (B, NU, NI),
           "calls": calls, "warmup": warmup, "peak_flops": PEAK,
           "not_measured": "other B, Adam / Adagrad / momentum, the SeqRec form, weights and offsets, host id lists"}
    for D in dims:
        forms = [dict(name=p, o=rt.Optimizer.sgd(0.05),
                      tables=(rt.Table(NU, D).init_uniform(seed=1), rt.Table(NI, D).init_uniform(seed=2), rt.Table(NI, 1).init_uniform(seed=3)))
                 for p in ("fp32", "bf16")]
        for S in cands:
            def ids():
                return (torch.randint(0, NU, (B,), dtype=torch.int32, device=dev), torch.randint(0, NI, (B,), dtype=torch.int32, device=dev),
                        torch.randint(0, NI, (S,), dtype=torch.int32, device=dev))

            def call(f, train=None):
                a = ids()
                torch.cuda.synchronize(); ctx.synchronize()
                t0 = time.perf_counter()
                rt.sampled_softmax_step(f["o"], *f["tables"], *a, train=train, want_loss=False, precision=f["name"])
                ctx.synchronize()
                return (time.perf_counter() - t0) * 1e6

            us = {f["name"]: [] for f in forms}
            for it in range(warmup + calls):        # interleaved: both forms see the same machine at the same time
                for f in forms:
                    dt = call(f)
                    if it >= warmup:
                        us[f["name"]].append(dt)
            geo = rt.sampled_softmax_geometry(B, S, D, precision="bf16")
            product = 2 * B * (-(-S // 64) * 64) * geo["dim"]
            res = {"geometry": geo, "flop_per_step": 5 * product}
            ctx.prof_enable(True)
            for f in forms:
                ctx.prof_reset(); call(f); st = ctx.prof_get()
                ctx.prof_reset(); call(f, train=("user",)); rw = ctx.prof_get()
                ctx.prof_reset(); rt.sampled_softmax_loss(*f["tables"], *ids(), precision=f["name"]); fw = ctx.prof_get()
                both, row, fwd = (x["gemm"]["total_ms"] * 1e3 for x in (st, rw, fw))
                t = us[f["name"]]
                kernels = {"row_side": row, "column_kernel": both - row, "forward_walk": fwd, "fused_slot": st["fused"]["total_ms"] * 1e3,
                           "other_slots": {k: v["total_ms"] * 1e3 for k, v in st.items() if k not in ("gemm", "fused") and v["launches"]}}
                if f["name"] == "bf16":
                    kernels["stats_walk"], kernels["query_gradient_walk"] = fwd, row - fwd
                res[f["name"]] = {"us_per_step_median": statistics.median(t), "us_per_step_spread": max(t) - min(t),
                                  "us_per_step": [round(x, 2) for x in t], "kernels_us_per_step": kernels,
                                  "fraction_of_peak_row_side": 3 * product / (row * 1e-6) / PEAK[f["name"]],
                                  "fraction_of_peak_step": 5 * product / (statistics.median(t) * 1e-6) / PEAK[f["name"]]}
            ctx.prof_enable(False)
            a, b = res["fp32"], res["bf16"]
            res["speedup_bf16"] = a["us_per_step_median"] / b["us_per_step_median"]
            res["row_side_bf16_faster"] = b["kernels_us_per_step"]["row_side"] < a["kernels_us_per_step"]["row_side"]
            out["D%d_S%d" % (D, S)] = res
        del forms
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cands", type=int, nargs="*", default=list(CANDS))
    ap.add_argument("--dims", type=int, nargs="*", default=[64, 128])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampled_softmax_bf16_bench.json"))
    ap.add_argument("--limit", type=int, default=300, help="seconds the measuring process may take")
    ap.add_argument("--measure", action="store_true", help="(the child) measure in this process and print one JSON line")
    a = ap.parse_args()
    if a.measure:
        print(json.dumps(measure(a.calls, a.warmup, a.cands, a.dims)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--measure", "--calls", str(a.calls),
           "--warmup", str(a.warmup), "--cands"] + [str(n) for n in a.cands] + ["--dims"] + [str(d) for d in a.dims]
    r = subprocess.run(cmd, capture_output=True, text=True)
    sys.stderr.write(r.stderr[-2000:])
    if r.returncode != 0:
        print("the measuring process failed with status %d" % r.returncode)
        return r.returncode
    doc = {"sampled_softmax_bf16": json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])}
    print(json.dumps(doc["sampled_softmax_bf16"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:            # one line per (D, S)
        fh.write('{"sampled_softmax_bf16": {\n' + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in doc["sampled_softmax_bf16"].items()) + "\n}}\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
