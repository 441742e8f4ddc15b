#!/usr/bin/env python3
"""The time of the full-softmax step with label sets (`rt.SeqRec.step_full(labels=...)`) at B = 4096, D = 64, bags and label sets
of 20, over 25 000 / 100 000 / 1 000 000 items under SGD, lists resident in HBM, no loss read-back -- beside the single-label
`rt.SeqRec.step_full` in the same process, the two interleaved call by call on tables of their own, a host clock around
synchronised calls; per form the median over the timed calls and their spread (max - min).  Without label sets the same labels
cost one sample per (user, label) pair: the single-label step at B * 20 samples is timed too where it fits the time limit
(--pairs).  After the timed calls one profiled step per form gives the profiling slots' totals (orx_prof_*): the new kernels sit in
"fused" (ls_prepare / ls_rows / ls_reduce / ls_query), "dedup" (the sort of the label entries) and "dup_apply" (ls_items), beside the
single-label step's own launches in those slots.  Each new kernel on its own comes from a kernel trace: run the measuring child
under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o b -- python scripts/multdae_bench.py --measure --items N
--pairs 0` and hand the kernel-stats csv to --trace-csv; its lines for the ls_ / fs_ / sort_ / bag_ kernels are copied into the
result as they are (both forms run in that process: the fs_ walks are counted for both).
--parent-tree DIR: a tree with the PARENT commit's package and library; the single-label step is then timed in child processes
that alternate between this tree and that one (A B A B), a median per process: the single-label kernels must not have become
slower.  The measuring processes run as children under time limits of their own; a failure ends the script.  Results go to
`--out`, profiles/multdae_bench.json.

    python scripts/multdae_bench.py [--calls 7] [--warmup 3] [--parent-tree DIR] [--out profiles/multdae_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, D, BAG, SET = 4096, 64, 20, 20
ITEMS = (25_000, 100_000, 1_000_000)


def med(us):
    return {"us_per_step_median": statistics.median(us), "us_per_step_spread": max(us) - min(us), "us_per_step": [round(t, 2) for t in us]}


def measure_single(calls, warmup, items):
    """the single-label step alone, with nothing this tree has and its parent lacks"""
    import torch
    from openrec_amd import runtime as rt
    torch.manual_seed(0)
    ctx = rt.default_context()
    dev = torch.device("cuda", ctx.device)
    out = {}
    ptr = torch.arange(0, (B + 1) * BAG, BAG, dtype=torch.int32, device=dev)
    for NI in items:
        net = rt.SeqRec(rt.Table(NI, D).init_uniform(seed=1), rt.Table(NI, D).init_uniform(seed=2), rt.Table(NI, 1).init_uniform(seed=3), pool="mean")
        o = rt.Optimizer.sgd(0.05)
        us = []
        for it in range(warmup + calls):
            bag = torch.randint(0, NI, (B * BAG,), dtype=torch.int32, device=dev)
            pid = torch.randint(0, NI, (B,), dtype=torch.int32, device=dev)
            torch.cuda.synchronize(); ctx.synchronize()
            t0 = time.perf_counter()
            net.step_full(o, (ptr, bag), pid, want_loss=False)
            ctx.synchronize()
            if it >= warmup:
                us.append((time.perf_counter() - t0) * 1e6)
        out["items_%d" % NI] = med(us)
        del net
        torch.cuda.empty_cache()
    return out


def measure(calls, warmup, items, pairs):
    import torch
    from openrec_amd import runtime as rt
    torch.manual_seed(0)
    ctx = rt.default_context()
    dev = torch.device("cuda", ctx.device)
    out = {"workload": "B=%d D=%d, bags of %d, label sets of %d, mean pooling, SGD, lists on the device, no read-back" % (B, D, BAG, SET),
           "calls": calls, "warmup": warmup,
           "not_measured": "other B and D, Adam / Adagrad / momentum, label weights, sample weights and item offsets, train masks, the tower form, "
                           "skewed label sets (an item in every set)"}
    ptr = torch.arange(0, (B + 1) * BAG, BAG, dtype=torch.int32, device=dev)
    lptr = torch.arange(0, (B + 1) * SET, SET, dtype=torch.int32, device=dev)
    pptr = torch.arange(0, (B * SET + 1) * BAG, BAG, dtype=torch.int32, device=dev) if pairs else None
    for NI in items:
        def tables():
            return rt.Table(NI, D).init_uniform(seed=1), rt.Table(NI, D).init_uniform(seed=2), rt.Table(NI, 1).init_uniform(seed=3)
        forms = [dict(name="single_label", net=rt.SeqRec(*tables(), pool="mean"), o=rt.Optimizer.sgd(0.05), us=[]),
                 dict(name="label_sets", net=rt.SeqRec(*tables(), pool="mean"), o=rt.Optimizer.sgd(0.05), us=[])]
        if pairs and NI <= pairs:
            forms.append(dict(name="single_label_one_sample_per_pair", net=rt.SeqRec(*tables(), pool="mean"), o=rt.Optimizer.sgd(0.05), us=[]))

        def step(f):
            bag = torch.randint(0, NI, (B * BAG,), dtype=torch.int32, device=dev)
            lab = torch.randint(0, NI, (B * SET,), dtype=torch.int32, device=dev)
            rep = bag.view(B, 1, BAG).expand(B, SET, BAG).reshape(-1).contiguous() if f["name"].endswith("pair") else None
            torch.cuda.synchronize(); ctx.synchronize()
            t0 = time.perf_counter()
            if f["name"] == "single_label":
                f["net"].step_full(f["o"], (ptr, bag), lab[:B], want_loss=False)
            elif f["name"] == "label_sets":
                f["net"].step_full(f["o"], (ptr, bag), labels=(lptr, lab), want_loss=False)
            else:
                f["net"].step_full(f["o"], (pptr, rep), lab, want_loss=False)
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e6

        for it in range(warmup + calls):                # interleaved: every form sees the same box at the same time
            for f in forms:
                dt = step(f)
                if it >= warmup:
                    f["us"].append(dt)
        res = {f["name"]: med(f["us"]) for f in forms}
        res["label_sets_over_single_label"] = res["label_sets"]["us_per_step_median"] / res["single_label"]["us_per_step_median"]
        ctx.prof_enable(True)
        slots = {}
        for f in forms[:2]:
            ctx.prof_reset()
            step(f)
            st = ctx.prof_get()
            slots[f["name"]] = {k: {"us": v["total_ms"] * 1e3, "launches": v["launches"]} for k, v in st.items() if v["launches"]}
        ctx.prof_enable(False)
        res["profiling_slots_us_one_step"] = slots
        res["slots_note"] = ("label sets add, per step: in 'fused' ls_prepare_kernel (in place of fs_prepare_kernel), ls_rows_kernel and "
                             "ls_reduce_kernel (in place of fs_finalize_kernel) and ls_query_kernel; in 'dedup' the radix sort of the label "
                             "entries; in 'dup_apply' ls_items_kernel; the 'gemm' slot is the three walks, the same kernels in both forms")
        out["items_%d" % NI] = res
        del forms
        torch.cuda.empty_cache()
    return out


def child(args, limit, tree=None):
    env = dict(os.environ)
    if tree:
        env["MULTDAE_BENCH_TREE"] = os.path.abspath(tree)
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, env=env)
    sys.stderr.write(r.stderr[-2000:])
    if r.returncode != 0:
        print("the measuring process failed with status %d" % r.returncode)
        sys.exit(r.returncode)
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--items", type=int, nargs="*", default=list(ITEMS))
    ap.add_argument("--pairs", type=int, default=100_000, help="time one sample per (user, label) pair up to this many items (0: never)")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--trace-csv", default=None, help="a kernel-stats csv of rocprofv3 over one run of this script, copied into the result")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multdae_bench.json"))
    ap.add_argument("--limit", type=int, default=300, help="seconds a measuring process may take")
    ap.add_argument("--measure", action="store_true", help="(a child) measure in this process and print one JSON line")
    ap.add_argument("--measure-single", action="store_true", help="(a child) the single-label step alone")
    a = ap.parse_args()
    sys.path.insert(0, os.environ.get("MULTDAE_BENCH_TREE") or ROOT)
    if a.measure:
        print(json.dumps(measure(a.calls, a.warmup, a.items, a.pairs)), flush=True)
        return 0
    if a.measure_single:
        print(json.dumps(measure_single(a.calls, a.warmup, a.items)), flush=True)
        return 0
    common = ["--calls", str(a.calls), "--warmup", str(a.warmup), "--items"] + [str(n) for n in a.items]
    doc = {"multdae_bench": child(["--measure", "--pairs", str(a.pairs)] + common, a.limit)}
    if a.parent_tree:
        runs = []
        for k in range(4):                              # A B A B: this build, the parent's, this build, the parent's
            which = "this_build" if k % 2 == 0 else "parent_build"
            runs.append({"build": which, **child(["--measure-single"] + common, a.limit, a.parent_tree if k % 2 else None)})
        doc["single_label_step_this_build_against_the_parent"] = {
            "what": "rt.SeqRec.step_full with one label per sample, the workload above, one process per entry in the order listed",
            "runs": runs}
    if a.trace_csv and os.path.exists(a.trace_csv):
        with open(a.trace_csv) as fh:
            doc["kernel_stats_csv"] = [ln.rstrip("\n") for ln in fh if any(k in ln for k in ("ls_", "fs_", "sort_", "bag_", "Name"))]
    print(json.dumps(doc))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
