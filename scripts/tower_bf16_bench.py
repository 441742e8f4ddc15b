#!/usr/bin/env python3
"""The tower step (`rt.DeepSeqRec.step_full`) at the four precision combinations -- precision= of the softmax x tower_precision=
of the layers -- on the shapes of scripts/tower_bench.py: B = 4096, Dh = 64, two side tables, bags of 20, lists resident in HBM, SGD,
no loss read-back, the layers 80 -> 256 -> 128 -> 64 and the single layer 80 -> 80, over 25 000 and 100 000 items.  One process, the
forms interleaved call by call on tables of their own, a host clock around synchronised calls; medians after warm-up, per
repetition, and the spread of the repetitions' medians.

The tower's kernels alone, from the dispatch-attached events (orx_prof_*; "gemm" and "fused" slots) by differences of profiled
calls at the same tower precision tp.  The layers' kernels do not depend on the item count, so this part runs over 1 000 items:
the softmax walks that the differences take out are then a few microseconds and not the milliseconds whose jitter would swamp
the tower's own times:
    cast      fused(user_table, tp=bf16) - fused(user_table, tp=fp32)      (the input launch is the same)
    forward   gemm(user_table)
    g         gemm(step, train=history) - forward - gemm(SeqRec step of the output dim, train=history)
    dW        gemm(step, train=history+tower) - gemm(step, train=history)          (fp32: g and dW are one kernel, reported as backward)
    finish    fused(step, train=history+tower) - fused(step, train=history)
and each product's rate as a fraction of the 2.5 PF bf16 dense peak (fp32 kernels: of the 157 TF fp32 matrix peak).  The
expectation checked: cast + forward + g + dW + finish in bf16 is below forward + backward + finish in fp32, by more than the
spread of the repetitions.  Then examples/youtube_rec_synthetic.py is run for 300 steps at both tower precisions.

    python scripts/tower_bf16_bench.py [--calls 7] [--warmup 3] [--reps 3] [--out profiles/tower_bf16_bench.json]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, DH, BAG, SIDE = 4096, 64, 20, ((2, 8), (1000, 8))
ITEMS = (25_000, 100_000)
KERNEL_ITEMS = 1000                             # the item count of the kernel-by-kernel part
TOWERS = {"ref_1_layer": (80, 80), "3_layers": (80, 256, 128, 64)}
PEAK_BF16, PEAK_FP32 = 2.5e15, 157e12
FORMS = [(p, tp) for p in ("fp32", "bf16") for tp in ("fp32", "bf16")]


def measure(calls, warmup, reps, items):
    import numpy as np
    import torch
    from openrec_amd import runtime as rt
    torch.manual_seed(0)
    ctx = rt.default_context()
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(0)
    out = {"workload": "B=%d Dh=%d, side tables %s, bags of %d (mean), lists on the device, SGD, no read-back" % (B, DH, SIDE, BAG),
           "calls": calls, "warmup": warmup, "reps": reps, "peak_bf16": PEAK_BF16, "peak_fp32": PEAK_FP32}

    def make_tower(NI, widths):
        H, V, b = (rt.Table(NI, d).init_uniform(seed=s) for d, s in ((DH, 1), (widths[-1], 2), (1, 3)))
        S = [rt.Table(r, d).init_uniform(seed=4 + j) for j, (r, d) in enumerate(SIDE)]
        layers = []
        for l in range(len(widths) - 1):
            a = (6.0 / (widths[l] + widths[l + 1])) ** 0.5
            W = rt.Table(widths[l], widths[l + 1]).write(rng.uniform(-a, a, (widths[l], widths[l + 1])).astype(np.float32))
            layers.append((W, rt.Table(1, widths[l + 1]).write(np.zeros((1, widths[l + 1]), np.float32))))
        return rt.DeepSeqRec(H, V, b, layers, side=S)

    def lists(NI):
        ptr = torch.arange(0, (B + 1) * BAG, BAG, dtype=torch.int32, device=dev)
        bag = torch.randint(0, NI, (B * BAG,), dtype=torch.int32, device=dev)
        pid = torch.randint(0, NI, (B,), dtype=torch.int32, device=dev)
        return ptr, bag, pid, tuple(torch.randint(0, r, (B,), dtype=torch.int32, device=dev) for r, _ in SIDE)

    def timed(fn):
        torch.cuda.synchronize(); ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e6

    def profiled(fn):
        ctx.prof_reset()
        timed(fn)
        got = {k: v["total_ms"] * 1e3 for k, v in ctx.prof_get().items() if v["launches"]}
        return got.get("gemm", 0.0), got.get("fused", 0.0)

    # ---- 1. the step at the four combinations, interleaved ------------------------------------------------------------------
    for NI in items:
        res = {}
        for name, widths in TOWERS.items():
            nets = {f: (make_tower(NI, widths), rt.Optimizer.sgd(0.05)) for f in FORMS}
            meds = {f: [] for f in FORMS}
            for _ in range(reps):
                us = {f: [] for f in FORMS}
                for it in range(warmup + calls):
                    ptr, bag, pid, f = lists(NI)
                    for (p, tp), (net, o) in nets.items():
                        dt = timed(lambda: net.step_full(o, (ptr, bag), pid, f, want_loss=False, precision=p, tower_precision=tp))
                        if it >= warmup:
                            us[(p, tp)].append(dt)
                for f in FORMS:
                    meds[f].append(statistics.median(us[f]))
            res[name] = {"softmax_%s_tower_%s" % f: {"us_median": statistics.median(m), "us_spread_of_medians": max(m) - min(m),
                                                      "us_medians": [round(x, 1) for x in m]} for f, m in meds.items()}
            del nets
            torch.cuda.empty_cache()
        out["items_%d" % NI] = res

    # ---- 2. the tower's kernels alone ---------------------------------------------------------------------------------------
    NI = KERNEL_ITEMS
    ptr, bag, pid, f = lists(NI)
    ctx.prof_enable(True)
    kern = {}
    for name, widths in TOWERS.items():
        macs = sum(widths[l] * widths[l + 1] for l in range(len(widths) - 1))
        seq = rt.SeqRec(rt.Table(NI, widths[-1]).init_uniform(seed=1), rt.Table(NI, widths[-1]).init_uniform(seed=2), rt.Table(NI, 1).init_uniform(seed=3))
        net, o, Q = make_tower(NI, widths), rt.Optimizer.sgd(0.05), rt.Table(B, widths[-1])
        runs = {"fp32": [], "bf16": []}
        for rep in range(reps + 1):                     # (the first repetition grows the scratch and is dropped)
            sq = profiled(lambda: seq.step_full(o, (ptr, bag), pid, train=("history",), want_loss=False))
            row = {}
            for tp in ("fp32", "bf16"):
                ut = profiled(lambda: net.user_table((ptr, bag), f, out=Q, tower_precision=tp))
                sh = profiled(lambda: net.step_full(o, (ptr, bag), pid, f, train=("history",), want_loss=False, tower_precision=tp))
                st = profiled(lambda: net.step_full(o, (ptr, bag), pid, f, train=("history", "tower"), want_loss=False, tower_precision=tp))
                row[tp] = dict(input_fused_us=ut[1], forward_us=ut[0], g_us=sh[0] - ut[0] - sq[0], dW_us=st[0] - sh[0], finish_us=st[1] - sh[1])
            row["bf16"]["cast_us"] = row["bf16"]["input_fused_us"] - row["fp32"]["input_fused_us"]
            row["fp32"]["cast_us"] = 0.0
            if rep:
                for tp in runs:
                    runs[tp].append(row[tp])
        k = {}
        for tp, rows in runs.items():
            k[tp] = {key: statistics.median(r[key] for r in rows) for key in ("cast_us", "forward_us", "g_us", "dW_us", "finish_us")}
            tot = [r["cast_us"] + r["forward_us"] + r["g_us"] + r["dW_us"] + r["finish_us"] for r in rows]
            k[tp]["tower_us"], k[tp]["tower_us_spread"], k[tp]["tower_us_reps"] = statistics.median(tot), max(tot) - min(tot), [round(x, 2) for x in tot]
            peak = PEAK_BF16 if tp == "bf16" else PEAK_FP32
            for key in ("forward_us", "g_us", "dW_us"):
                k[tp][key[:-3] + "_fraction_of_peak"] = 2 * B * macs / (k[tp][key] * 1e-6) / peak if k[tp][key] > 0 else None
        k["bf16_over_fp32"] = k["bf16"]["tower_us"] / k["fp32"]["tower_us"]
        k["bf16_is_faster_beyond_the_spread"] = bool(k["fp32"]["tower_us"] - k["bf16"]["tower_us"] > max(k["fp32"]["tower_us_spread"], k["bf16"]["tower_us_spread"]))
        k["note"] = "fp32: g_us + dW_us are tower_backward_kernel, one launch per layer that computes both; its split by training mask is nominal"
        kern[name] = k
        del net, seq
    ctx.prof_enable(False)
    out["kernels_at_items_%d" % NI] = kern
    return out


def example(tp, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, "examples", "youtube_rec_synthetic.py"), "--steps", "300",
           "--tower-precision", tp]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        return None
    last = r.stdout.strip().splitlines()[-1]
    m = re.search(r"loss ([\d.]+) .*recall@(\d+) tower ([\d.]+)", last)
    return {"steps": 300, "loss": float(m.group(1)), "k": int(m.group(2)), "recall": float(m.group(3))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--items", type=int, nargs="*", default=list(ITEMS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tower_bf16_bench.json"))
    ap.add_argument("--limit", type=int, default=400, help="seconds the measuring process may take")
    ap.add_argument("--measure", action="store_true", help="(the child) measure in this process and print one JSON line")
    a = ap.parse_args()
    if a.measure:
        print(json.dumps(measure(a.calls, a.warmup, a.reps, a.items)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--measure", "--calls", str(a.calls),
           "--warmup", str(a.warmup), "--reps", str(a.reps), "--items"] + [str(n) for n in a.items]
    r = subprocess.run(cmd, capture_output=True, text=True)
    sys.stderr.write(r.stderr[-3000:])
    if r.returncode != 0:
        print("the measuring process failed with status %d" % r.returncode)
        return r.returncode
    doc = {"tower_bf16": json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])}
    doc["tower_bf16"]["example_300_steps"] = {}
    for tp in ("fp32", "bf16"):
        got = example(tp, 200)
        if got is None:
            print("the example failed at tower precision %s" % tp)
            return 1
        doc["tower_bf16"]["example_300_steps"][tp] = got
    print(json.dumps(doc["tower_bf16"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
