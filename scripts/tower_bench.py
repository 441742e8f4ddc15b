#!/usr/bin/env python3
"""The time of the tower step (`rt.DeepSeqRec.step_full`) at B = 4096 over 25 000 / 100 000 / 1 000 000 items: history table of
dim 64, two side tables (2 and 1000 rows, d = 8), bags of 20, lists resident in HBM, SGD, no loss read-back -- with the reference's
single layer (80 -> 80) and with the layers 80 -> 256 -> 128 -> 64 -- against `rt.SeqRec.step_full` (D = 64) on the same lists,
the path without a tower.  One process, the forms of one item count interleaved call by call on tables of their own, a host
clock around synchronised calls; per form the median over the timed calls and their spread.

The tower's kernels alone, from the dispatch-attached events (orx_prof_*), at 100 000 items:
    input, forward     one profiled `user_table`: the "fused" slot is tower_input, the "gemm" slot the forward launches
    backward           gemm(step, train=tower) - gemm(user_table) - gemm(SeqRec of the tower's output dim, train=history): what is
                       left of the step's matrix-core time once the forward and the full softmax's two walks are taken out
    finish             fused(step, train=tower) - fused(that SeqRec step) + fused(rt.bag_pool) - input
    side applies       orx_apply_rows on a 2-row and on a 1000-row table of dim 8 with 4096 ids, gradient rows of stride 80, each
                       alone (every slot of the call, the sort included), and a host clock around the synchronised call
and as fractions of the 157 TF fp32 matrix peak (forward: 2 B sum K_l N_l; backward: twice that) and of the float4-copy rate
(`Context.copy_bandwidth`; input: the bytes of the gathered rows and of x0).  Also the same tower forward and backward in torch
(`embedding_bag`, `embedding`, `cat`, `linear`, `relu`, autograd to every parameter, no softmax), and `user_table` at B = 65536.
The measuring process runs as a child under a time limit of its own; a failure ends the script.

    python scripts/tower_bench.py [--calls 7] [--warmup 3] [--out profiles/tower_bench.json]
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

B, DH, BAG, SIDE = 4096, 64, 20, ((2, 8), (1000, 8))
ITEMS = (25_000, 100_000, 1_000_000)
TOWERS = {"ref_1_layer": (80, 80), "3_layers": (80, 256, 128, 64)}
PEAK = 157e12                                 # fp32 MFMA, MI355X


def measure(calls, warmup, items):
    import numpy as np
    import torch
    from openrec_amd import runtime as rt
    torch.manual_seed(0)
    ctx = rt.default_context()
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(0)
    out = {"workload": "B=%d Dh=%d, side tables %s, bags of %d (mean), lists on the device, SGD, no read-back" % (B, DH, SIDE, BAG),
           "calls": calls, "warmup": warmup, "peak_flops": PEAK,
           "not_measured": "other B, Adam / Adagrad / momentum, weights and item offsets, host lists"}

    def med(us):
        return {"us_median": statistics.median(us), "us_spread": max(us) - min(us), "us": [round(t, 2) for t in us]}

    def make_tower(NI, widths):
        H = rt.Table(NI, DH).init_uniform(seed=1)
        V = rt.Table(NI, widths[-1]).init_uniform(seed=2)
        b = rt.Table(NI, 1).init_uniform(seed=3)
        S = [rt.Table(r, d).init_uniform(seed=4 + j) for j, (r, d) in enumerate(SIDE)]
        layers = []
        for l in range(len(widths) - 1):
            a = (6.0 / (widths[l] + widths[l + 1])) ** 0.5
            W = rt.Table(widths[l], widths[l + 1]).write(rng.uniform(-a, a, (widths[l], widths[l + 1])).astype(np.float32))
            layers.append((W, rt.Table(1, widths[l + 1]).write(np.zeros((1, widths[l + 1]), np.float32))))
        return rt.DeepSeqRec(H, V, b, layers, side=S)

    def make_seq(NI, D):
        return rt.SeqRec(rt.Table(NI, D).init_uniform(seed=1), rt.Table(NI, D).init_uniform(seed=2), rt.Table(NI, 1).init_uniform(seed=3))

    def lists(NI, n=B):
        ptr = torch.arange(0, (n + 1) * BAG, BAG, dtype=torch.int32, device=dev)
        bag = torch.randint(0, NI, (n * BAG,), dtype=torch.int32, device=dev)
        pid = torch.randint(0, NI, (n,), dtype=torch.int32, device=dev)
        f = tuple(torch.randint(0, r, (n,), dtype=torch.int32, device=dev) for r, _ in SIDE)
        return ptr, bag, pid, f

    def timed(fn):
        torch.cuda.synchronize(); ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e6

    def profiled(fn):
        ctx.prof_reset()
        timed(fn)
        return {k: v["total_ms"] * 1e3 for k, v in ctx.prof_get().items() if v["launches"]}

    copy_rate = ctx.copy_bandwidth(1 << 28, 5) * 1e9          # (GB/s, read + write)
    out["copy_bytes_per_s"] = copy_rate

    # ---- 1. the step against SeqRec.step_full -----------------------------------------------------------------------------
    for NI in items:
        forms = [dict(name="seqrec", net=make_seq(NI, DH), o=rt.Optimizer.sgd(0.05), us=[])]
        for name, widths in TOWERS.items():
            forms.append(dict(name="tower_" + name, net=make_tower(NI, widths), o=rt.Optimizer.sgd(0.05), us=[]))
        for it in range(warmup + calls):            # interleaved: every form sees the same box at the same time
            ptr, bag, pid, f = lists(NI)
            for fm in forms:
                if fm["name"] == "seqrec":
                    dt = timed(lambda: fm["net"].step_full(fm["o"], (ptr, bag), pid, want_loss=False))
                else:
                    dt = timed(lambda: fm["net"].step_full(fm["o"], (ptr, bag), pid, f, want_loss=False))
                if it >= warmup:
                    fm["us"].append(dt)
        res = {fm["name"]: med(fm["us"]) for fm in forms}
        for name in TOWERS:
            res["tower_" + name]["over_seqrec"] = res["tower_" + name]["us_median"] / res["seqrec"]["us_median"]
        out["items_%d" % NI] = res
        del forms
        torch.cuda.empty_cache()

    # ---- 2. the tower's kernels alone -----------------------------------------------------------------------------------------
    NI = 100_000 if 100_000 in items else items[0]
    ptr, bag, pid, f = lists(NI)
    ctx.prof_enable(True)
    kern = {}
    for name, widths in TOWERS.items():
        net, seq = make_tower(NI, widths), make_seq(NI, widths[-1])
        o = rt.Optimizer.sgd(0.05)
        Q = rt.Table(B, widths[-1])
        pool_out = rt.Table(B, DH)
        for _ in range(2):                          # (the first call of each kind grows the scratch)
            ut = profiled(lambda: net.user_table((ptr, bag), f, out=Q))
            st = profiled(lambda: net.step_full(o, (ptr, bag), pid, f, train=("tower",), want_loss=False))
            sq = profiled(lambda: seq.step_full(o, (ptr, bag), pid, train=("history",), want_loss=False))
            bp = profiled(lambda: rt.bag_pool(net.H, (ptr, bag), pool_out))
            full = profiled(lambda: net.step_full(o, (ptr, bag), pid, f, want_loss=False))
        macs = sum(widths[l] * widths[l + 1] for l in range(len(widths) - 1))
        k = {"input_us": ut["fused"], "forward_us": ut["gemm"],
             "backward_us": st["gemm"] - ut["gemm"] - sq["gemm"],
             "finish_us": st["fused"] - sq["fused"] + bp["fused"] - ut["fused"],
             "bag_pool_us": bp["fused"], "step_all_slots_us": full, "step_all_slots_total_us": sum(full.values())}
        k["tower_launches_us"] = k["input_us"] + k["forward_us"] + k["backward_us"] + k["finish_us"]
        k["forward_fraction_of_peak"] = 2 * B * macs / (k["forward_us"] * 1e-6) / PEAK
        k["backward_fraction_of_peak"] = 4 * B * macs / (k["backward_us"] * 1e-6) / PEAK
        in_bytes = B * (BAG * DH + sum(d for _, d in SIDE) + widths[0]) * 4
        k["input_fraction_of_copy_rate"] = in_bytes / (k["input_us"] * 1e-6) / copy_rate
        kern[name] = k
        del net, seq
    # the side applies, each alone: orx_apply_rows with gradient rows of stride 80
    g = torch.randn(B, 80, device=dev) * 1e-3
    o = rt.Optimizer.sgd(0.05)
    ctx.after_torch(g, *f)
    for (rows, d), ids in zip(SIDE, f):
        t = rt.Table(rows, d).init_uniform(seed=9)
        call = lambda: rt.check(ctx._lib.orx_apply_rows(ctx._h, o._h, t._h, None, ids.data_ptr(), B, g.data_ptr(), 80))
        call(); ctx.synchronize()
        slots = profiled(call)
        ctx.prof_enable(False)
        us = [timed(call) for _ in range(calls)]
        ctx.prof_enable(True)
        kern["side_apply_%d_rows" % rows] = {"kernels_us": slots, "kernels_total_us": sum(slots.values()), "host_clock": med(us)}
    ctx.prof_enable(False)
    out["kernels_at_items_%d" % NI] = kern
    for name in TOWERS:
        step_us = out["items_%d" % NI]["tower_" + name]["us_median"]
        kern[name]["tower_share_of_step"] = kern[name]["tower_launches_us"] / step_us
    for n_items in items:
        for name in TOWERS:
            out["items_%d" % n_items]["tower_" + name]["tower_share_of_step"] = \
                kern[name]["tower_launches_us"] / out["items_%d" % n_items]["tower_" + name]["us_median"]

    # ---- 3. the same tower forward and backward in torch ------------------------------------------------------------------------
    tor = {}
    for name, widths in TOWERS.items():
        H = (torch.rand(NI, DH, device=dev) * 0.1 - 0.05).requires_grad_()
        S = [(torch.rand(r, d, device=dev) * 0.1 - 0.05).requires_grad_() for r, d in SIDE]
        Ws = [(torch.randn(widths[l + 1], widths[l], device=dev) * 0.1).requires_grad_() for l in range(len(widths) - 1)]
        cs = [torch.zeros(widths[l + 1], device=dev, requires_grad=True) for l in range(len(widths) - 1)]
        gq = torch.randn(B, widths[-1], device=dev)
        off = ptr[:-1].long()

        def fwd_bwd():
            x = torch.cat([torch.nn.functional.embedding(fj.long(), Sj) for fj, Sj in zip(f, S)] +
                          [torch.nn.functional.embedding_bag(bag.long(), H, off, mode="mean")], 1)
            for W, c in zip(Ws, cs):
                x = torch.relu(torch.nn.functional.linear(x, W, c))
            torch.autograd.grad(x, [H] + S + Ws + cs, gq)
            torch.cuda.synchronize()
        us = [timed(fwd_bwd) for _ in range(warmup + calls)][warmup:]
        tor[name] = med(us)
        tor[name]["note"] = "the history gradient is a dense [items, Dh] tensor here (embedding_bag without sparse=True)"
    out["torch_tower_forward_backward"] = tor

    # ---- 4. serving: user_table at B = 65536 ---------------------------------------------------------------------------------
    nb = 65536
    ptr, bag, pid, f = lists(NI, nb)
    serve = {}
    for name, widths in TOWERS.items():
        net = make_tower(NI, widths)
        Q = rt.Table(nb, widths[-1])
        us = [timed(lambda: net.user_table((ptr, bag), f, out=Q)) for _ in range(warmup + calls)][warmup:]
        serve[name] = med(us)
        serve[name]["geometry"] = rt.tower_geometry(nb, widths)
    out["user_table_B65536"] = serve
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--items", type=int, nargs="*", default=list(ITEMS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tower_bench.json"))
    ap.add_argument("--limit", type=int, default=400, help="seconds the measuring process may take")
    ap.add_argument("--measure", action="store_true", help="(the child) measure in this process and print one JSON line")
    a = ap.parse_args()
    if a.measure:
        print(json.dumps(measure(a.calls, a.warmup, a.items)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--measure", "--calls", str(a.calls),
           "--warmup", str(a.warmup), "--items"] + [str(n) for n in a.items]
    r = subprocess.run(cmd, capture_output=True, text=True)
    sys.stderr.write(r.stderr[-3000:])
    if r.returncode != 0:
        print("the measuring process failed with status %d" % r.returncode)
        return r.returncode
    doc = {"tower_step": json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])}
    print(json.dumps(doc["tower_step"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
