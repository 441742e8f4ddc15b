#!/usr/bin/env python3
"""The time and the memory of the full-softmax step (`rt.fullsoftmax_step`, `rt.SeqRec.step_full`) at B = 4096, D = 64 over
25 000 / 100 000 / 1 000 000 items, under SGD and Adam, in the user-table form and the SeqRec form (bags of 20), ids resident in
HBM, no loss read-back.  Two yardsticks in the same run: (a) the same step written in torch (`q @ V.T + b`, `cross_entropy`,
autograd, a dense SGD update of V and b) with its peak memory from `torch.cuda.max_memory_allocated` -- it stores the B x items
logit matrix and its gradient, and does three products where this route does five and stores none, so it may well be faster
where its matrix fits --; (b) `rt.multineg_step("softmax", N = 64)` at the same B, a DIFFERENT objective, for context.
One process, the forms of one item count interleaved call by call on tables of their own, a host clock around synchronised
calls; per form the median over the timed calls and their spread (max - min).  After the timed calls one profiled step and one
profiled forward per form give the kernels' own times from the dispatch-attached events (orx_prof_*): the MFMA walks sit in the
"gemm" slot (the LSE walk alone is read from the forward), prepare / item copy / finalize / finish in "fused"; and the achieved
fraction of the 157 TF fp32 matrix peak on the count 5 * 2 * B * NIp * Dp.  The measuring process runs as a child under a time
limit of its own; a failure ends the script.  Results go to `--out`, profiles/fullsoftmax_bench.json.

    python scripts/fullsoftmax_bench.py [--calls 7] [--warmup 3] [--out profiles/fullsoftmax_bench.json]
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

B, D, NU, BAG = 4096, 64, 100_000, 20
ITEMS = (25_000, 100_000, 1_000_000)
PEAK = 157e12                                 # fp32 MFMA, MI355X


def measure(calls, warmup, items):
    import torch
    from openrec_amd import runtime as rt
    torch.manual_seed(0)
    ctx = rt.default_context()
    dev = torch.device("cuda", ctx.device)
    out = {"workload": "B=%d D=%d, ids on the device, no read-back; SeqRec form: bags of %d, mean pooling" % (B, D, BAG),
           "calls": calls, "warmup": warmup, "peak_flops": PEAK,
           "note": "multineg_softmax_N64: a different objective (64 drawn negatives), quoted as a yardstick only; torch: the same "
                   "objective through a stored B x items matrix, SGD on V and b, the query rows fixed",
           "not_measured": "other B and D, Adagrad / momentum, weights and item offsets, train masks"}

    def med(us):
        return {"us_per_step_median": statistics.median(us), "us_per_step_spread": max(us) - min(us), "us_per_step": [round(t, 2) for t in us]}

    for NI in items:
        geo = rt.fullsoftmax_geometry(B, NI, D)
        forms = []
        for optname in ("sgd", "adam"):
            for kind in ("user", "seqrec"):
                first = rt.Table(NU if kind == "user" else NI, D).init_uniform(seed=1)
                tV = rt.Table(NI, D).init_uniform(seed=2); tb = rt.Table(NI, 1).init_uniform(seed=3)
                o = rt.Optimizer.sgd(0.05) if optname == "sgd" else rt.Optimizer.adam(0.001)
                forms.append(dict(name=f"{kind}_{optname}", kind=kind, tables=(first, tV, tb), o=o, us=[],
                                  net=rt.SeqRec(first, tV, tb, pool="mean") if kind == "seqrec" else None))
        mn = dict(name="multineg_softmax_N64", kind="multineg", o=rt.Optimizer.sgd(0.05), us=[],
                  tables=(rt.Table(NU, D).init_uniform(seed=1), rt.Table(NI, D).init_uniform(seed=2), rt.Table(NI, 1).init_uniform(seed=3)))
        forms.append(mn)
        tq = {"name": "torch_sgd", "kind": "torch", "us": []}
        try:
            tq["Q"] = torch.rand(NU, D, device=dev) * 0.1 - 0.05
            tq["V"] = (torch.rand(NI, D, device=dev) * 0.1 - 0.05).requires_grad_()
            tq["b"] = (torch.rand(NI, device=dev) * 0.1 - 0.05).requires_grad_()
            forms.append(tq)
        except torch.cuda.OutOfMemoryError:
            tq = None
        ptr = torch.arange(0, (B + 1) * BAG, BAG, dtype=torch.int32, device=dev)

        def step(f, profiled_forward=False):
            uid = torch.randint(0, NU, (B,), dtype=torch.int32, device=dev)
            pid = torch.randint(0, NI, (B,), dtype=torch.int32, device=dev)
            bag = torch.randint(0, NI, (B * BAG,), dtype=torch.int32, device=dev) if f["kind"] == "seqrec" else None
            nid = torch.randint(0, NI, (B, 64), dtype=torch.int32, device=dev) if f["kind"] == "multineg" else None
            torch.cuda.synchronize(); ctx.synchronize()
            t0 = time.perf_counter()
            if f["kind"] == "user":
                if profiled_forward:
                    rt.fullsoftmax_loss(*f["tables"], uid, pid)
                else:
                    rt.fullsoftmax_step(f["o"], *f["tables"], uid, pid, want_loss=False)
            elif f["kind"] == "seqrec":
                if profiled_forward:
                    f["net"].loss_full((ptr, bag), pid)
                else:
                    f["net"].step_full(f["o"], (ptr, bag), pid, want_loss=False)
            elif f["kind"] == "multineg":
                rt.multineg_step("softmax", f["o"], *f["tables"], uid, pid, nid, want_loss=False)
            else:
                q = f["Q"][uid.long()]
                loss = torch.nn.functional.cross_entropy(q @ f["V"].T + f["b"][None, :], pid.long())
                gV, gb = torch.autograd.grad(loss, (f["V"], f["b"]))
                with torch.no_grad():
                    f["V"].sub_(0.05 * gV); f["b"].sub_(0.05 * gb)
                torch.cuda.synchronize()
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e6

        torch_failed = None
        for it in range(warmup + calls):            # interleaved: every form sees the same box at the same time
            for f in list(forms):
                if f["kind"] == "torch" and it == 0:
                    torch.cuda.reset_peak_memory_stats()
                    f["base_bytes"] = torch.cuda.memory_allocated()
                try:
                    dt = step(f)
                except torch.cuda.OutOfMemoryError as e:
                    if f["kind"] != "torch":
                        raise
                    torch_failed = str(e)[:200]
                    forms.remove(f)
                    continue
                if f["kind"] == "torch" and it == 0:
                    f["peak_bytes"] = torch.cuda.max_memory_allocated() - f["base_bytes"]
                if it >= warmup:
                    f["us"].append(dt)
        res = {"geometry": geo, "scratch_bytes": geo["scratch_bytes"], "matrix_bytes_2BNI4": 2 * B * NI * 4,
               "flop_per_step": 5 * 2 * B * (-(-NI // 64) * 64) * geo["dim"]}
        for f in forms:
            res[f["name"]] = med(f["us"])
        if tq is not None and tq in forms:
            res["torch_sgd"]["peak_bytes_beyond_the_tables"] = tq["peak_bytes"]
        else:
            res["torch_sgd"] = {"did_not_fit": torch_failed or "out of memory at set-up"}
        # the kernels' own times: one profiled step and one profiled forward per form
        ctx.prof_enable(True)
        for f in (f for f in forms if f["kind"] in ("user", "seqrec")):
            ctx.prof_reset()
            step(f)
            st = ctx.prof_get()
            ctx.prof_reset()
            step(f, profiled_forward=True)
            fw = ctx.prof_get()
            lse_us, walks_us = fw["gemm"]["total_ms"] * 1e3, st["gemm"]["total_ms"] * 1e3
            r = res[f["name"]]
            r["kernels_us_per_step"] = {
                "lse_walk": lse_us, "gradient_walks_both_sides": walks_us - lse_us, "fused_slot": st["fused"]["total_ms"] * 1e3,
                "other_slots": {k: v["total_ms"] * 1e3 for k, v in st.items() if k not in ("gemm", "fused") and v["launches"]}}
            r["fraction_of_peak_lse_walk"] = res["flop_per_step"] / 5 / (lse_us * 1e-6) / PEAK
            r["fraction_of_peak_gradient_walks"] = res["flop_per_step"] * 4 / 5 / ((walks_us - lse_us) * 1e-6) / PEAK
            r["fraction_of_peak_walks"] = res["flop_per_step"] / (walks_us * 1e-6) / PEAK
            r["fraction_of_peak_step"] = res["flop_per_step"] / (r["us_per_step_median"] * 1e-6) / PEAK
        ctx.prof_enable(False)
        out["items_%d" % NI] = res
        del forms, tq, mn
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--items", type=int, nargs="*", default=list(ITEMS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fullsoftmax_bench.json"))
    ap.add_argument("--limit", type=int, default=400, help="seconds the measuring process may take")
    ap.add_argument("--measure", action="store_true", help="(the child) measure in this process and print one JSON line")
    a = ap.parse_args()
    if a.measure:
        print(json.dumps(measure(a.calls, a.warmup, a.items)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--measure", "--calls", str(a.calls),
           "--warmup", str(a.warmup), "--items"] + [str(n) for n in a.items]
    r = subprocess.run(cmd, capture_output=True, text=True)
    sys.stderr.write(r.stderr[-2000:])
    if r.returncode != 0:
        print("the measuring process failed with status %d" % r.returncode)
        return r.returncode
    doc = {"fullsoftmax_step": json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])}
    print(json.dumps(doc["fullsoftmax_step"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
