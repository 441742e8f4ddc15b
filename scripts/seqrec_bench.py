#!/usr/bin/env python3
"""The time of the history-pooled sequence recommender's train step and of its pooling kernel (`rt.SeqRec`, `rt.bag_pool`): 1M
items, D = 64, B = 65536 histories per step, bags of 20 and of 50 uniform items (n = 1.3M / 3.3M list entries), N = 16 negatives,
sampled softmax, ragged lists on the device, no loss read-back.

  step        milliseconds per step, SGD and Adam, and its split from the library's own kernel timestamps (`ctx.prof_enable`):
              the pool alone (`bag_pool` into a table), the gradient launch (the fused class of a step minus the pool), and, from
              steps that train the history table alone / the item table alone, the sort of bag_items with the owner rewrite, the
              history apply (with the scaling of g_q), the item apply (its sort included)
  pool        the pooling kernel's rate in gathered bytes n * D * 4 against the float4-copy rate `ctx.copy_bandwidth` measures in
              the same process, and against `rt.graph_spmm` over a device CSR that holds the same lists, timed interleaved
  torch       the same step written in torch (embedding_bag, autograd, index_add_), SGD, timed interleaved with the library's
              step, repetition by repetition.  Measurement only: the package never imports it

Every figure is the median of `--reps` repetitions after `--warmup`, timed by device events on the stream the library runs on.
The measuring process runs as a child under a time limit of its own.  Results go to `--out`, profiles/seqrec_bench.json.

    python scripts/seqrec_bench.py [--reps 10] [--warmup 3] [--out profiles/seqrec_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NI, D, B, N = 1_000_000, 64, 65536, 16
BAGS = (20, 50)


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

    H = rt.Table(NI, D, ctx=ctx).init_uniform(seed=1); V = rt.Table(NI, D, ctx=ctx).init_uniform(seed=2)
    b = rt.Table(NI, 1, ctx=ctx).init_uniform(seed=3)
    Q = rt.Table(B, D, ctx=ctx); Qs = rt.Table(B, D, ctx=ctx)
    net = rt.SeqRec(H, V, b, pool="mean")
    copy_gbs = ctx.copy_bandwidth()
    out = dict(items=NI, dim=D, batch=B, negatives=N, loss="softmax", pool="mean", copy_GBs=copy_gbs, reps=reps, warmup=warmup)
    rng = np.random.default_rng(3)
    kw = dict(loss="softmax", l2_reg=1e-4, want_loss=False)
    for L in BAGS:
        n = B * L
        ptr_h = (np.arange(B + 1, dtype=np.int64) * L).astype(np.int32)
        items_h = rng.integers(0, NI, n).astype(np.int32)
        with torch.cuda.stream(stream):
            ptr, items = torch.from_numpy(ptr_h).to(dv), torch.from_numpy(items_h).to(dv)
            pid = torch.from_numpy(rng.integers(0, NI, B).astype(np.int32)).to(dv)
            nid = torch.from_numpy(rng.integers(0, NI, (B, N)).astype(np.int32)).to(dv)
            stream.synchronize()
        bags = (ptr, items)
        res = dict(bag_len=L, n=n)

        # ---- (a) the step and its split
        for name, mk in (("sgd", lambda: rt.Optimizer.sgd(lr=0.05, ctx=ctx)), ("adam", lambda: rt.Optimizer.adam(lr=0.001, ctx=ctx))):
            o = mk()
            res["step_" + name], = timed(lambda: net.step(o, bags, pid, nid, **kw))
            ctx.prof_enable(True)
            kp = kernel_ms(lambda: rt.bag_pool(H, bags, Q, pool="mean"))
            kh = kernel_ms(lambda: net.step(o, bags, pid, nid, train=("history",), **kw))
            ki = kernel_ms(lambda: net.step(o, bags, pid, nid, train=("item", "bias"), **kw))
            ctx.prof_enable(False)
            res["split_" + name] = dict(pool_ms=kp["fused"], gradient_ms=kh["fused"] - kp["fused"], sort_ms=kh["dedup"],
                                        history_apply_ms=kh["dup_apply"], item_apply_ms=sum(v for k, v in ki.items() if k not in ("fused", "loss_reduce")),
                                        item_classes={k: v for k, v in ki.items() if v > 0})

        # ---- (b) the pool against the copy rate and against graph_spmm over the same lists
        csr = rt.ALSCsr(ptr_h.astype(np.int64), items_h, None, NI).to_device(ctx)
        tp, tg = timed(lambda: rt.bag_pool(H, bags, Q, pool="sum"), lambda: rt.graph_spmm(H, Qs, csr, long_segments=0))
        gathered = n * D * 4
        for t in (tp, tg):
            t.update(bytes=gathered, GBs=gathered / t["ms_median"] / 1e6, of_copy_rate=gathered / t["ms_median"] / 1e6 / copy_gbs)
        res["pool"], res["graph_spmm"] = tp, tg
        res["pool_over_graph_spmm_time"] = tp["ms_median"] / tg["ms_median"]
        res["pool_equals_graph_spmm"] = bool(np.array_equal(Q.read(0, 4096), Qs.read(0, 4096)))

        # ---- (c) the same step in torch, interleaved with the library's
        lr = 0.05
        with torch.cuda.stream(stream):
            Ht = torch.from_numpy(H.read()).to(dv); Vt = torch.from_numpy(V.read()).to(dv); bt = torch.from_numpy(b.read()).to(dv).reshape(-1)
            i64, off64, p64, n64 = items.long(), ptr[:-1].long(), pid.long(), nid.long().reshape(-1)

            def torch_step():
                h = Ht.index_select(0, i64).requires_grad_(True)        # (autograd of embedding_bag's weight would be dense: 1M x 64)
                q = torch.nn.functional.embedding_bag(torch.arange(n, device=dv), h, off64, mode="mean")
                p = Vt.index_select(0, p64).requires_grad_(True); ng = Vt.index_select(0, n64).requires_grad_(True)
                bp = bt.index_select(0, p64).requires_grad_(True); bn = bt.index_select(0, n64).requires_grad_(True)
                sp = (q * p).sum(1) + bp
                sn = (q[:, None, :] * ng.view(B, N, D)).sum(2) + bn.view(B, N)
                J = (torch.logsumexp(torch.cat([sp[:, None], sn], 1), 1) - sp).mean() \
                    + 1e-4 * 0.5 * ((q * q).sum() + (p * p).sum() + (ng * ng).sum())
                gh, gp, gn, gbp, gbn = torch.autograd.grad(J, (h, p, ng, bp, bn))
                Ht.index_add_(0, i64, gh, alpha=-lr)
                Vt.index_add_(0, p64, gp, alpha=-lr); Vt.index_add_(0, n64, gn, alpha=-lr)
                bt.index_add_(0, p64, gbp, alpha=-lr); bt.index_add_(0, n64, gbn, alpha=-lr)
            stream.synchronize()
        o1 = rt.Optimizer.sgd(lr=lr, ctx=ctx)
        t1, tt = timed(lambda: net.step(o1, bags, pid, nid, **kw), torch_step)
        res["one_step_sgd"], res["torch_step_sgd"] = t1, tt
        res["torch_over_library"] = tt["ms_median"] / t1["ms_median"]
        del Ht, Vt, bt, csr
        out[f"bags_of_{L}"] = res
    ctx.check_index_error()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seqrec_bench.json"))
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
    print(f"copy rate {round(res['copy_GBs'])} GB/s")
    for L in BAGS:
        r = res[f"bags_of_{L}"]
        print(f"bags of {L}: step sgd {r['step_sgd']['ms_median']:.3f} ms, adam {r['step_adam']['ms_median']:.3f} ms; torch "
              f"{r['torch_step_sgd']['ms_median']:.3f} ms ({r['torch_over_library']:.2f}x the library's)")
        print("   split sgd: " + ", ".join(f"{k} {v:.3f}" for k, v in r["split_sgd"].items() if k != "item_classes"))
        print(f"   pool {r['pool']['ms_median']:.3f} ms = {r['pool']['of_copy_rate']:.3f} of the copy rate; graph_spmm "
              f"{r['graph_spmm']['ms_median']:.3f} ms = {r['graph_spmm']['of_copy_rate']:.3f}; same bits: {r['pool_equals_graph_spmm']}")


if __name__ == "__main__":
    main()
