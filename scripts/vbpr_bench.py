#!/usr/bin/env python3
"""The time of the VBPR train step and of serving its item table (`rt.VBPR`): 1M users x 1M items, latent width Dl = 32, projection
width Dc = 32, features of dim Fd = 512 (2 GB of fp32 in HBM), B = 65536 triplets per step, K = 20 steps per call, ids on the device,
no loss read-back.

  step          microseconds per step of a K-step call, SGD and Adam
  kernels       each of the step's three kernels alone, from the library's own kernel timestamps (`ctx.prof_enable`): the projection
                is the matrix-core time of a step that trains the user table alone (no projection gradient is computed), the pass
                over the triplets the fused class of any step, the projection gradient the matrix-core time of a step that trains the
                projection alone minus the projection's
  feature pass  the projection and the projection gradient each gather F[pid] and F[nid] once: 2 B Fd 4 algorithmic bytes per pass,
                over the kernel's time, as a fraction of the float4-copy rate `ctx.copy_bandwidth` measures in the same process
  bpr           the plain BPR K-step (`rt.pairwise_step`) at D = 64 on tables of the same size: what the content half costs
  torch         the same VBPR step written in torch (index_select, mm, autograd, index_add_), SGD, timed interleaved with the
                library's one-step call, repetition by repetition.  Measurement only: the package never imports it
  item_table    `item_table()` for all 1M items (a copy of V and one projection of every feature row)

Every figure is the median of `--reps` repetitions after `--warmup`, timed by device events on the stream the library runs on.
The measuring process runs as a child under a time limit of its own.  Results go to `--out`, profiles/vbpr_bench.json.

    python scripts/vbpr_bench.py [--reps 10] [--warmup 3] [--out profiles/vbpr_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NU = NI = 1_000_000
DL = DC = 32
FD, B, K = 512, 65536, 20


def measure(reps, warmup):
    import numpy as np
    import torch
    from openrec_amd import runtime as rt
    stream = torch.cuda.Stream()
    ctx = rt.Context(0, stream=stream.cuda_stream)          # the library's work on a stream torch's events can time
    dv = torch.device("cuda", 0)

    def timed(*fns):
        """the fns interleaved, repetition by repetition -> one dict per fn"""
        ts = [[] for _ in fns]
        with torch.cuda.stream(stream):
            for it in range(warmup + reps):
                for k, fn in enumerate(fns):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream); fn(); e1.record(stream)
                    e1.synchronize()
                    if it >= warmup:
                        ts[k].append(e0.elapsed_time(e1))
        return [dict(ms_median=statistics.median(t), ms_spread=max(t) - min(t), ms=[round(x, 3) for x in t]) for t in ts]

    def kernel_ms(fn):
        """per call of fn, the library's kernel time by class (median over the repetitions)"""
        rows = []
        for it in range(warmup + reps):
            ctx.prof_reset()
            fn()
            ctx.synchronize()
            if it >= warmup:
                rows.append({k: v["total_ms"] for k, v in ctx.prof_get().items()})
        return {k: statistics.median(r[k] for r in rows) for k in rows[0]}

    with torch.cuda.stream(stream):
        Ft = torch.randn((NI, FD), device=dv, dtype=torch.float32)
        rng = np.random.default_rng(3)
        uid, pid, nid = (torch.from_numpy(rng.integers(0, n, (K, B)).astype(np.int32)).to(dv) for n in (NU, NI, NI))
        stream.synchronize()
    feats = rt.ItemFeatures(Ft, ctx=ctx)
    U = rt.Table(NU, DL + DC, ctx=ctx).init_uniform(seed=1); V = rt.Table(NI, DL, ctx=ctx).init_uniform(seed=2)
    b = rt.Table(NI, 1, ctx=ctx).init_uniform(seed=3); E = rt.Table(FD, DC, ctx=ctx).init_uniform(seed=4)
    net = rt.VBPR(U, V, b, E, feats)
    copy_gbs = ctx.copy_bandwidth()
    out = dict(users=NU, items=NI, latent_dim=DL, proj_dim=DC, feature_dim=FD, batch=B, steps_per_call=K, copy_GBs=copy_gbs,
               geometry=rt.vbpr_geometry(B, FD, DC), reps=reps, warmup=warmup)
    kw = dict(l2_reg=1e-4, l2_proj=1e-4, want_loss=False)

    # ---- the K-step call, and the plain BPR K-step at D = 64 beside it
    Ub = rt.Table(NU, 64, ctx=ctx).init_uniform(seed=5); Vb = rt.Table(NI, 64, ctx=ctx).init_uniform(seed=6)
    bb = rt.Table(NI, 1, ctx=ctx).init_uniform(seed=7)
    for name, mk in (("sgd", lambda: rt.Optimizer.sgd(lr=0.05, ctx=ctx)), ("adam", lambda: rt.Optimizer.adam(lr=0.001, ctx=ctx))):
        ov, ob = mk(), mk()
        tv, tb = timed(lambda: net.step(ov, uid, pid, nid, K=K, **kw),
                       lambda: rt.pairwise_step("bpr", ob, Ub, Vb, bb, uid, pid, nid, K=K, want_loss=False))
        for t in (tv, tb):
            t["us_per_step"] = t["ms_median"] * 1e3 / K
        out["step_" + name], out["bpr_d64_step_" + name] = tv, tb
        out[f"vbpr_over_bpr_{name}"] = tv["ms_median"] / tb["ms_median"]
    del Ub, Vb, bb

    # ---- the three kernels alone
    ctx.prof_enable(True)
    osgd = rt.Optimizer.sgd(lr=0.05, ctx=ctx)
    ka = kernel_ms(lambda: net.step(osgd, uid[0], pid[0], nid[0], train=("user",), **kw))
    kb = kernel_ms(lambda: net.step(osgd, uid[0], pid[0], nid[0], train=("proj",), **kw))
    ctx.prof_enable(False)
    pass_bytes = 2 * B * FD * 4
    proj_ms, pair_ms, dproj_ms = ka["gemm"], ka["fused"], kb["gemm"] - ka["gemm"]
    out["kernel_project"] = dict(ms=proj_ms, bytes=pass_bytes, GBs=pass_bytes / proj_ms / 1e6, of_copy_rate=pass_bytes / proj_ms / 1e6 / copy_gbs,
                                 gflops=2.0 * B * FD * DC / proj_ms / 1e6)
    out["kernel_pairs"] = dict(ms=pair_ms)
    out["kernel_dproj"] = dict(ms=dproj_ms, bytes=pass_bytes, GBs=pass_bytes / dproj_ms / 1e6, of_copy_rate=pass_bytes / dproj_ms / 1e6 / copy_gbs,
                               gflops=2.0 * B * FD * DC / dproj_ms / 1e6, finish_ms=kb["loss_reduce"])
    out["feature_passes_bytes"] = 2 * pass_bytes

    # ---- the same step in torch, interleaved with the library's one-step call
    lr = 0.05
    with torch.cuda.stream(stream):
        Ut = torch.from_numpy(U.read()).to(dv); Vt = torch.from_numpy(V.read()).to(dv); bt = torch.from_numpy(b.read()).to(dv).reshape(-1)
        Et = torch.from_numpy(E.read()).to(dv)
        u64, p64, n64 = uid[0].long(), pid[0].long(), nid[0].long()

        def torch_step():
            u = Ut.index_select(0, u64).requires_grad_(True)
            p = Vt.index_select(0, p64).requires_grad_(True); n = Vt.index_select(0, n64).requires_grad_(True)
            bp = bt.index_select(0, p64).requires_grad_(True); bn = bt.index_select(0, n64).requires_grad_(True)
            Ew = Et.detach().requires_grad_(True)
            delta = (Ft.index_select(0, p64) - Ft.index_select(0, n64)).mm(Ew)
            x = (u[:, :DL] * (p - n)).sum(1) + (u[:, DL:] * delta).sum(1) + bp - bn
            J = torch.nn.functional.softplus(-x.clamp(min=-30.0)).mean() + 1e-4 * 0.5 * ((u * u).sum() + (p * p).sum() + (n * n).sum()) \
                + 1e-4 * 0.5 * (Ew * Ew).sum()
            gu, gp, gn, gbp, gbn, gE = torch.autograd.grad(J, (u, p, n, bp, bn, Ew))
            Ut.index_add_(0, u64, gu, alpha=-lr)
            Vt.index_add_(0, p64, gp, alpha=-lr); Vt.index_add_(0, n64, gn, alpha=-lr)
            bt.index_add_(0, p64, gbp, alpha=-lr); bt.index_add_(0, n64, gbn, alpha=-lr)
            Et.add_(gE, alpha=-lr)
        stream.synchronize()
    o1 = rt.Optimizer.sgd(lr=lr, ctx=ctx)
    t1, tt = timed(lambda: net.step(o1, uid[0], pid[0], nid[0], **kw), torch_step)
    out["one_step_sgd"], out["torch_step_sgd"] = t1, tt
    out["torch_over_library"] = tt["ms_median"] / t1["ms_median"]

    # ---- serving: the item table of all items
    def table():
        net.invalidate()
        net.item_table()
    out["item_table"], = timed(table)
    tbytes = NI * (FD * 4 + DL * 4 + (DL + DC) * 4)
    out["item_table"].update(bytes=tbytes, of_copy_rate=tbytes / out["item_table"]["ms_median"] / 1e6 / copy_gbs)
    ctx.check_index_error()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vbpr_bench.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(measure(args.reps, args.warmup)))
        return
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--warmup", str(args.warmup)],
                       capture_output=True, text=True, timeout=500)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit(r.returncode)
    res = json.loads(next(line for line in r.stdout.splitlines() if line.startswith("RESULT "))[7:])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for k in ("step_sgd", "step_adam", "bpr_d64_step_sgd", "bpr_d64_step_adam"):
        print(f"{k:22s} {res[k]['us_per_step']:9.1f} us per step")
    for k in ("kernel_project", "kernel_pairs", "kernel_dproj"):
        print(f"{k:22s} {res[k]['ms'] * 1e3:9.1f} us" + (f"   {res[k]['of_copy_rate']:.3f} of the copy rate" if "of_copy_rate" in res[k] else ""))
    print(f"one step sgd {res['one_step_sgd']['ms_median']:.3f} ms, torch {res['torch_step_sgd']['ms_median']:.3f} ms; item table "
          f"{res['item_table']['ms_median']:.3f} ms ({res['item_table']['of_copy_rate']:.3f} of the copy rate); copy rate {round(res['copy_GBs'])} GB/s")


if __name__ == "__main__":
    main()
