#!/usr/bin/env python3
"""The time of the sampled-softmax step over a shared candidate list (`rt.sampled_softmax_step`) at 1M users x 1M items, D = 64,
B = 4096 and S in {1024, 8192}, SGD, ids resident in HBM, no loss read-back.  Two yardsticks in the same run, interleaved call
by call on tables of their own: `rt.fullsoftmax_step` (every item a column) and `rt.multineg_step("softmax", N = 64)` (64
negatives gathered per sample) -- different objectives, quoted for context.  One process, a host clock around synchronised
calls; per form the median over the timed calls and their spread (max - min).  After the timed calls one profiled step per S
gives the kernels' own times from the dispatch-attached events (orx_prof_*): the row kernel and the column kernel sit in the
"gemm" slot (the row kernel alone is read from a step with train=("user",)), gather and finish in "fused"; and the achieved
fraction of the 157 TF fp32 matrix peak on the count 2 B Sp Dp per product: 3 in the row kernel (S twice, G once), 2 in the
column kernel.  The measuring process runs as a child under a time limit of its own; a failure ends the script.  Results go to
`--out`, profiles/sampled_softmax_bench.json.

    python scripts/sampled_softmax_bench.py [--calls 9] [--warmup 3] [--out profiles/sampled_softmax_bench.json]
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

B, D, NU, NI = 4096, 64, 1_000_000, 1_000_000
CANDS = (1024, 8192)
PEAK = 157e12                                 # fp32 MFMA, MI355X


def measure(calls, warmup, cands, full):
    import torch
    from openrec_amd import runtime as rt
    torch.manual_seed(0)
    ctx = rt.default_context()
    dev = torch.device("cuda", ctx.device)
    out = {"workload": "B=%d D=%d, %d users x %d items, SGD, ids on the device, no read-back" % (B, D, NU, NI),
           "calls": calls, "warmup": warmup, "peak_flops": PEAK,
           "note": "fullsoftmax and multineg_softmax_N64 are different objectives, quoted as yardsticks only",
           "not_measured": "other B and D, Adam / Adagrad / momentum, the SeqRec form, weights and offsets, host id lists"}

    def med(us):
        return {"us_per_step_median": statistics.median(us), "us_per_step_spread": max(us) - min(us), "us_per_step": [round(t, 2) for t in us]}

    def tables():
        return (rt.Table(NU, D).init_uniform(seed=1), rt.Table(NI, D).init_uniform(seed=2), rt.Table(NI, 1).init_uniform(seed=3))

    forms = [dict(name="sampled_S%d" % S, kind="sampled", S=S, tables=tables(), o=rt.Optimizer.sgd(0.05), us=[]) for S in cands]
    forms.append(dict(name="multineg_softmax_N64", kind="multineg", tables=tables(), o=rt.Optimizer.sgd(0.05), us=[]))
    if full:
        forms.append(dict(name="fullsoftmax", kind="full", tables=tables(), o=rt.Optimizer.sgd(0.05), us=[]))

    def step(f, train=None):
        uid = torch.randint(0, NU, (B,), dtype=torch.int32, device=dev)
        pid = torch.randint(0, NI, (B,), dtype=torch.int32, device=dev)
        cand = torch.randint(0, NI, (f["S"],), dtype=torch.int32, device=dev) if f["kind"] == "sampled" else None
        nid = torch.randint(0, NI, (B, 64), dtype=torch.int32, device=dev) if f["kind"] == "multineg" else None
        torch.cuda.synchronize(); ctx.synchronize()
        t0 = time.perf_counter()
        if f["kind"] == "sampled":
            rt.sampled_softmax_step(f["o"], *f["tables"], uid, pid, cand, train=train, want_loss=False)
        elif f["kind"] == "multineg":
            rt.multineg_step("softmax", f["o"], *f["tables"], uid, pid, nid, want_loss=False)
        else:
            rt.fullsoftmax_step(f["o"], *f["tables"], uid, pid, want_loss=False)
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e6

    for it in range(warmup + calls):            # interleaved: every form sees the same box at the same time
        for f in forms:
            dt = step(f)
            if it >= warmup:
                f["us"].append(dt)
    for f in forms:
        out[f["name"]] = med(f["us"])
    # the kernels' own times: one profiled step, and one with the user table alone trained (no column kernel)
    ctx.prof_enable(True)
    for f in (f for f in forms if f["kind"] == "sampled"):
        geo = rt.sampled_softmax_geometry(B, f["S"], D)
        ctx.prof_reset(); step(f); st = ctx.prof_get()
        ctx.prof_reset(); step(f, train=("user",)); rw = ctx.prof_get()
        row_us, both_us = rw["gemm"]["total_ms"] * 1e3, st["gemm"]["total_ms"] * 1e3
        product = 2 * B * (-(-f["S"] // 64) * 64) * geo["dim"]
        r = out[f["name"]]
        r["geometry"] = geo
        r["flop_per_step"] = 5 * product
        r["kernels_us_per_step"] = {"row_kernel": row_us, "column_kernel": both_us - row_us, "fused_slot": st["fused"]["total_ms"] * 1e3,
                                    "other_slots": {k: v["total_ms"] * 1e3 for k, v in st.items() if k not in ("gemm", "fused") and v["launches"]}}
        r["fraction_of_peak_row_kernel"] = 3 * product / (row_us * 1e-6) / PEAK
        r["fraction_of_peak_column_kernel"] = 2 * product / ((both_us - row_us) * 1e-6) / PEAK
        r["fraction_of_peak_step"] = 5 * product / (r["us_per_step_median"] * 1e-6) / PEAK
    ctx.prof_enable(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cands", type=int, nargs="*", default=list(CANDS))
    ap.add_argument("--no-full", action="store_true", help="leave the full softmax out of the comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampled_softmax_bench.json"))
    ap.add_argument("--limit", type=int, default=300, help="seconds the measuring process may take")
    ap.add_argument("--measure", action="store_true", help="(the child) measure in this process and print one JSON line")
    a = ap.parse_args()
    if a.measure:
        print(json.dumps(measure(a.calls, a.warmup, a.cands, not a.no_full)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--measure", "--calls", str(a.calls),
           "--warmup", str(a.warmup), "--cands"] + [str(n) for n in a.cands] + (["--no-full"] if a.no_full else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    sys.stderr.write(r.stderr[-2000:])
    if r.returncode != 0:
        print("the measuring process failed with status %d" % r.returncode)
        return r.returncode
    doc = {"sampled_softmax_step": json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])}
    print(json.dumps(doc["sampled_softmax_step"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
