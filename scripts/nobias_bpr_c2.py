"""Biased against bias-free BPR at C2 (D = 64, 1M x 1M, B = 65 536, K = 20 per call, device ids, no loss read-back): one process,
calls alternating between the two forms, SGD and lazy Adam.  Prints the median wall-clock time per step of each form (a host clock
around synchronised calls).  profiles/nobias_bpr_c2.txt has the numbers and how they were taken.

    python scripts/nobias_bpr_c2.py [--calls 6] [--warmup 2] [--opts sgd,adam]
    python scripts/nobias_bpr_c2.py --kernels <rocprofv3 output dir>      per-launch medians of the fused / tail kernels of a
                                                                          `rocprofv3 --kernel-trace --stats` run of this script
    python scripts/nobias_bpr_c2.py --counters <rocprofv3 output dir>     bytes per launch of a `--pmc FETCH_SIZE` (or WRITE_SIZE)
                                                                          `--kernel-trace --output-format csv` run (one counter a run)
"""
import argparse
import csv
import glob
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NU = NI = 1_000_000
D, B, K = 64, 65536, 20
BYTES = {"bias-free": 1548, "biased": 1564}         # algorithmic bytes per triplet at D = 64 (SGD)


def timed(calls, warmup, opts):
    import torch
    from openrec_amd import runtime as rt
    torch.manual_seed(0)
    forms = []
    for opt_name in opts:
        for form in ("biased", "bias-free"):
            tU = rt.Table(NU, D).init_uniform(seed=1); tV = rt.Table(NI, D).init_uniform(seed=2)
            tb = rt.Table(NI, 1).init_uniform(seed=3) if form == "biased" else None
            opt = rt.Optimizer.sgd(0.05) if opt_name == "sgd" else rt.Optimizer.adam(0.001)
            rt.pairwise_reserve(opt, tU, tV, tb, K, B)
            forms.append(dict(opt=opt_name, form=form, tables=(tU, tV, tb), o=opt, times=[]))
    ctx = rt.default_context()
    for it in range(warmup + calls):
        for f in forms:
            ids = [torch.randint(0, n, (K, B), dtype=torch.int32, device="cuda") for n in (NU, NI, NI)]
            torch.cuda.synchronize(); ctx.synchronize()
            t0 = time.perf_counter()
            rt.pairwise_step("bpr", f["o"], *f["tables"], *ids, K=K, B=B, want_loss=False)
            ctx.synchronize()
            dt = (time.perf_counter() - t0) / K * 1e6
            if it >= warmup:
                f["times"].append(dt)
    for f in forms:
        print("%-5s %-9s median %.1f us/step   (%s)" % (f["opt"], f["form"], statistics.median(f["times"]),
                                                   " ".join("%.1f" % t for t in f["times"])))


def _line(name, v):
    med = statistics.median(v)
    line = "%8.2f us  %5d launches  %s" % (med, len(v), name)
    m = re.search(r"fused_kernel<(\d+), (\d+), (\d+), (\d+)", name)
    if m and m.group(3) == "0" and m.group(4) == "0":            # SGD, exact mode: the byte counts above
        mb = BYTES["bias-free" if m.group(2) == "16" else "biased"] * B / 1e6
        line += "   %.1f MB -> %.2f TB/s = %.3f of 8 TB/s" % (mb, mb / med, mb / med / 8.0)
    return line


def kernels(outdir):
    """per-launch medians from the trace database(s) rocprofv3 wrote under `outdir`"""
    import sqlite3
    rows = {}
    for fn in glob.glob(os.path.join(outdir, "**", "*.db"), recursive=True):
        for name, t0, t1 in sqlite3.connect(fn).execute("select name, start, end from kernels"):
            if "fused_kernel" in name or "tail_kernel" in name:
                rows.setdefault(name, []).append((t1 - t0) / 1e3)
    for name, v in sorted(rows.items()):
        print(_line(name, v))


def counters(outdir):
    """mean per launch of each counter of a `rocprofv3 --pmc <counter> --kernel-trace --output-format csv` run (FETCH_SIZE and
    WRITE_SIZE are in KB)"""
    acc = {}
    for fn in glob.glob(os.path.join(outdir, "**", "*counter_collection.csv"), recursive=True):
        with open(fn) as fh:
            for r in csv.DictReader(fh):
                if "fused_kernel" in r["Kernel_Name"]:
                    acc.setdefault((r["Kernel_Name"], r["Counter_Name"]), []).append(float(r["Counter_Value"]))
    for (name, ctr), v in sorted(acc.items()):
        print("%-12s %10.1f MB per launch (%d launches)  %s" % (ctr, statistics.mean(v) / 1e3, len(v), name))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--opts", default="sgd,adam")
    ap.add_argument("--kernels", default=None)
    ap.add_argument("--counters", default=None)
    a = ap.parse_args()
    if a.kernels:
        kernels(a.kernels)
    elif a.counters:
        counters(a.counters)
    else:
        timed(a.calls, a.warmup, a.opts.split(","))
