#!/usr/bin/env python3
"""The cost of per-triplet weights in the fused pairwise step at C2 (BPR, D = 64, 1M x 1M, B = 65 536, K = 20 per call, SGD, ids
and weights resident in HBM, no loss read-back): one process, calls alternating between `rt.pairwise_step(...)` and
`rt.pairwise_step(..., weights=w, l2_reg=0.01)` on tables of their own, a host clock around synchronised calls.  Per form the
median time per step over the timed calls and their spread (max - min), and the ratio of the medians.  The measuring process
runs as a child under a time limit of its own; a failure ends the script.  Results go to `--out` (a JSON file that is updated
in place: the keys "weighted_step" and, with --bench-lines, "bench" -- bench.py result lines of two builds, given as
label=file pairs, for the record that the plain entry points kept their time).  profiles/weighted_step_bench.json is that file.

    python scripts/weighted_step_bench.py [--calls 9] [--warmup 5] [--out profiles/weighted_step_bench.json]
    python scripts/weighted_step_bench.py --bench-lines parent=a.jsonl this=b.jsonl --out profiles/weighted_step_bench.json
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
D, B, K = 64, 65536, 20
BYTES = 3 * 256 * 2 + 2 * 4 * 2 + 12          # algorithmic bytes per triplet of the plain step (scripts/subset_bench.py); the weight adds 4


def measure(calls, warmup):
    import torch
    from openrec_amd import runtime as rt
    torch.manual_seed(0)
    ctx = rt.default_context()
    forms = []
    for name in ("unweighted", "weighted"):
        tU = rt.Table(NU, D).init_uniform(seed=1); tV = rt.Table(NI, D).init_uniform(seed=2); tb = rt.Table(NI, 1).init_uniform(seed=3)
        opt = rt.Optimizer.sgd(0.05)
        rt.pairwise_reserve(opt, tU, tV, tb, K, B)
        forms.append(dict(name=name, tables=(tU, tV, tb), o=opt, us=[]))

    def call(f):
        ids = [torch.randint(0, n, (K, B), dtype=torch.int32, device="cuda") for n in (NU, NI, NI)]
        kw = dict(weights=torch.rand((K, B), dtype=torch.float32, device="cuda") * 2, l2_reg=0.01) if f["name"] == "weighted" else {}
        torch.cuda.synchronize(); ctx.synchronize()
        t0 = time.perf_counter()
        rt.pairwise_step("bpr", f["o"], *f["tables"], *ids, K=K, B=B, want_loss=False, **kw)
        ctx.synchronize()
        return (time.perf_counter() - t0) / K * 1e6

    for it in range(warmup + calls):            # interleaved: both forms see the same box at the same time
        for f in forms:
            dt = call(f)
            if it >= warmup:
                f["us"].append(dt)
    out = {"workload": "BPR D=%d %dx%d B=%d K=%d SGD, ids and weights on the device, no read-back" % (D, NU, NI, B, K),
           "calls": calls, "warmup": warmup, "algorithmic_bytes_per_triplet": {"unweighted": BYTES, "weighted": BYTES + 4}}
    for f in forms:
        out[f["name"]] = {"us_per_step_median": statistics.median(f["us"]), "us_per_step_spread": max(f["us"]) - min(f["us"]),
                          "us_per_step": [round(t, 2) for t in f["us"]]}
    out["ratio_weighted_over_unweighted"] = out["weighted"]["us_per_step_median"] / out["unweighted"]["us_per_step_median"]
    out["spread_over_median_unweighted"] = out["unweighted"]["us_per_step_spread"] / out["unweighted"]["us_per_step_median"]
    return out


def bench_lines(pairs):
    """label=file pairs of bench.py output -> {label: {"lines": [...], "ms_per_step": [...], "kernel_us": [...], medians}}"""
    res = {}
    for pair in pairs:
        label, fn = pair.split("=", 1)
        lines = []
        for ln in open(fn):
            ln = ln.strip()
            if ln.startswith("{") and "ms_per_step" in ln:
                lines.append(json.loads(ln))
        ms = [x["ms_per_step"] for x in lines]
        ku = [x.get("roofline", {}).get("kernel_us") for x in lines]
        res[label] = {"lines": lines, "ms_per_step": ms, "kernel_us": ku, "ms_per_step_median": statistics.median(ms),
                      "kernel_us_median": statistics.median(ku) if all(k is not None for k in ku) else None,
                      "ms_per_step_spread": max(ms) - min(ms), "kernel_us_spread": (max(ku) - min(ku)) if all(k is not None for k in ku) else None}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_step_bench.json"))
    ap.add_argument("--limit", type=int, default=300, help="seconds the measuring process may take")
    ap.add_argument("--bench-lines", nargs="*", default=None)
    ap.add_argument("--measure", action="store_true", help="(the child) measure in this process and print one JSON line")
    a = ap.parse_args()
    if a.measure:
        print(json.dumps(measure(a.calls, a.warmup)), flush=True)
        return 0
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.bench_lines is not None:
        doc.setdefault("bench", {}).update(bench_lines(a.bench_lines))
    else:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--measure", "--calls", str(a.calls), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            print("the measuring process failed with status %d" % r.returncode)
            return r.returncode
        doc["weighted_step"] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        print(json.dumps(doc["weighted_step"]))
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
