"""Full step against the users-only step at C2 (BPR, D = 64, 1M x 1M, B = 65 536, K = 20 per call, ids resident in HBM, no
loss read-back): one process, calls alternating between the two forms, SGD and lazy Adam.  Per form: the median wall-clock time
per step (a host clock around synchronised calls, profiling off) and, from a second round with the library's own event
profiling on (orx_prof_*: HIP events on the kernels' own dispatches), the median device time per step summed over every kernel
class the step launches.  profiles/subset_bpr_c2.txt has the numbers and how they were taken.

    python scripts/subset_bench.py [--calls 6] [--warmup 5] [--opts sgd,adam] [--no-prof]
    python scripts/subset_bench.py --trace <dir>      per-launch medians and the idle time in front of each launch, from the
                                                      kernel-trace csv of a `rocprofv3 --kernel-trace --stats --output-format csv
                                                      -d <dir> -- python scripts/subset_bench.py --opts sgd --no-prof` run
"""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NU = NI = 1_000_000
D, B, K = 64, 65536, 20
# algorithmic bytes per triplet at D = 64, SGD.  Full step: 3 rows and 2 biases read and written, 3 ids read.  Users only, the
# gradient launch: 3 rows, 2 biases and 3 ids read, one gradient row written; its apply: the gradient row and its sorted (row,
# position) pair read, the user row read and written -- the route as built moves MORE bytes than the full step
BYTES = {"full": 3 * 256 * 2 + 2 * 4 * 2 + 12, "users_grads": 3 * 256 + 2 * 4 + 12 + 256, "users_apply": 256 + 8 + 2 * 256}


def run(calls, warmup, opts, prof=True):
    import torch
    from openrec_amd import runtime as rt
    torch.manual_seed(0)
    forms = []
    for opt_name in opts:
        for form, train in (("full", None), ("users", ("user",))):
            tU = rt.Table(NU, D).init_uniform(seed=1); tV = rt.Table(NI, D).init_uniform(seed=2); tb = rt.Table(NI, 1).init_uniform(seed=3)
            opt = rt.Optimizer.sgd(0.05) if opt_name == "sgd" else rt.Optimizer.adam(0.001)
            rt.pairwise_reserve(opt, tU, tV, tb, K, B)
            forms.append(dict(opt=opt_name, form=form, train=train, tables=(tU, tV, tb), o=opt, wall=[], dev=[], classes={}))
    ctx = rt.default_context()

    def call(f):
        ids = [torch.randint(0, n, (K, B), dtype=torch.int32, device="cuda") for n in (NU, NI, NI)]
        torch.cuda.synchronize(); ctx.synchronize()
        t0 = time.perf_counter()
        rt.pairwise_step("bpr", f["o"], *f["tables"], *ids, K=K, B=B, want_loss=False, train=f["train"])
        ctx.synchronize()
        return (time.perf_counter() - t0) / K * 1e6

    for it in range(warmup + calls):            # wall clock, profiling off
        for f in forms:
            dt = call(f)
            if it >= warmup:
                f["wall"].append(dt)
    ctx.prof_enable(prof)
    for it in range(1 + calls if prof else 0):                 # device time of the kernels (one more warm-up call with the events on)
        for f in forms:
            ctx.prof_reset()
            call(f)
            got = ctx.prof_get()
            if it >= 1:
                f["dev"].append(sum(v["total_ms"] for v in got.values()) * 1e3 / K)
                for name, v in got.items():
                    if v["launches"]:
                        f["classes"].setdefault(name, []).append((v["total_ms"] * 1e3 / K, v["launches"] / K))
    ctx.prof_enable(False)
    print("BPR D=%d %dx%d B=%d K=%d, ids on the device, %d timed calls per form after %d warm-up calls" % (D, NU, NI, B, K, calls, warmup))
    med = {}
    for f in forms:
        w, d = statistics.median(f["wall"]), statistics.median(f["dev"]) if f["dev"] else float("nan")
        med[(f["opt"], f["form"])] = (w, d)
        print("%-5s %-6s step %.1f us (median; %s)   kernels %.1f us (median; %s)" % (
            f["opt"], f["form"], w, " ".join("%.1f" % t for t in f["wall"]), d, " ".join("%.1f" % t for t in f["dev"])))
        for name, v in sorted(f["classes"].items()):
            print("      %-12s %.2f us/step  %.1f launches/step" % (name, statistics.median(x[0] for x in v), statistics.median(x[1] for x in v)))
    for opt_name in opts:
        (wf, df), (wu, du) = med[(opt_name, "full")], med[(opt_name, "users")]
        print("%-5s users-only / full: step %.3f, kernels %.3f" % (opt_name, wu / wf, du / df))
    print("algorithmic bytes per triplet (SGD): full %d; users only %d = gradient launch %d + apply %d" % (
        BYTES["full"], BYTES["users_grads"] + BYTES["users_apply"], BYTES["users_grads"], BYTES["users_apply"]))


def trace(outdir):
    """which launch costs the step its time: per kernel name the median duration and the median idle time of the device in front
    of it (its start minus the end of the launch before it), over the launches whose predecessor is a step kernel too"""
    rows = []
    for fn in glob.glob(os.path.join(outdir, "**", "*kernel_trace.csv"), recursive=True):
        with open(fn) as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    step = ("fused_kernel", "subset_pair_grads", "csr_apply", "csr_finish", "tail_kernel")
    short = lambda n: next((k for k in step if k in n), None)
    acc = {}
    for (s0, e0, n0), (s1, e1, n1) in zip(rows, rows[1:]):
        a, b = short(n0), short(n1)
        if a is None or b is None:
            continue
        d = acc.setdefault((a, b), dict(dur=[], gap=[]))
        d["dur"].append((e1 - s1) / 1e3); d["gap"].append((s1 - e0) / 1e3)
    print("%d kernel records" % len(rows))
    for (a, b), d in sorted(acc.items(), key=lambda kv: -len(kv[1]["dur"])):
        if len(d["dur"]) >= 20:
            print("%-18s after %-18s %6d launches  kernel %7.2f us  idle before it %7.2f us (medians)" % (
                b, a, len(d["dur"]), statistics.median(d["dur"]), statistics.median(d["gap"])))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--opts", default="sgd,adam")
    ap.add_argument("--no-prof", action="store_true", help="skip the round with the library's event profiling on")
    ap.add_argument("--trace", default=None)
    a = ap.parse_args()
    if a.trace:
        trace(a.trace)
    else:
        run(a.calls, a.warmup, a.opts.split(","), prof=not a.no_prof)
