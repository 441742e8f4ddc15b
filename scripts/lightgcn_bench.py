#!/usr/bin/env python3
"""The time of LightGCN's propagation and train step (`rt.graph_spmm`, `rt.LightGCN`) on the set of scripts/als_bench.py: 1M users x
1M items, 20M records (about 18.1M distinct observations), items ~ Zipf(1.05), users uniform, D = 64, L = 3, both CSRs and the
scale vectors resident in HBM.

  half-layer   one `graph_spmm` over all rows with the layer sum fused (acc given), in the user direction (rows = users, short
               even rows) and in the item direction (rows = items, skewed: the longest row is cut into segments); algorithmic
               bytes nnz (4 D + 8) + rows 4 D 3 over the time, as a fraction of the float4-copy rate `ctx.copy_bandwidth`
               measures in the same process
  control      the same half-layer on a set whose items are drawn uniformly (even rows, no popular rows for the caches to hold):
               what the skewed rows of the item direction cost is its time per byte against this one's
  propagate    the 2 L half-layers and the two layer-0 scalings of `LightGCN.propagate`
  yardstick    the same propagation by `torch.sparse.mm` on CSR tensors whose values already carry the edge weights (so it
               needs no scaling pass), with the layer sums as torch adds; timed interleaved with `propagate`, repetition by
               repetition.  Measurement only: the package never imports it.  If torch cannot run it, that is recorded.
  step         `LightGCN.step` at B = 65536, SGD and Adam, ids on the device, no loss read-back

Every figure is the median of `--reps` repetitions after `--warmup`, timed by device events on the stream the library runs on.
The measuring process runs as a child under a time limit of its own.  Results go to `--out`, profiles/lightgcn_bench.json.

    python scripts/lightgcn_bench.py [--reps 10] [--warmup 3] [--out profiles/lightgcn_bench.json]
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
NNZ = 20_000_000
D, L, B = 64, 3, 65536


def records(zipf=True, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    users = rng.integers(0, NU, NNZ, dtype=np.int64)
    if zipf:
        cdf = np.cumsum(np.arange(1, NI + 1, dtype=np.float64) ** -1.05)
        cdf /= cdf[-1]
        items = rng.permutation(NI)[np.searchsorted(cdf, rng.random(NNZ))]
    else:
        items = rng.integers(0, NI, NNZ, dtype=np.int64)
    rec = np.zeros(NNZ, dtype=[("user_id", np.int32), ("item_id", np.int32)])
    rec["user_id"], rec["item_id"] = users, items
    return rec


def measure(reps, warmup):
    import numpy as np
    import torch
    from openrec_amd import runtime as rt
    stream = torch.cuda.Stream()
    ctx = rt.Context(0, stream=stream.cuda_stream)          # the library's work on a stream torch's events can time

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

    graph = rt.InteractionGraph(records(), NU, NI, norm="sym", ctx=ctx)
    nnz = graph.nnz
    U = rt.Table(NU, D, ctx=ctx).init_uniform(seed=1); V = rt.Table(NI, D, ctx=ctx).init_uniform(seed=2)
    copy_gbs = ctx.copy_bandwidth()
    out = dict(users=NU, items=NI, nnz=nnz, dim=D, layers=L, batch=B, segment_len=rt.graph_segment_len(), copy_GBs=copy_gbs,
               reps=reps, warmup=warmup)

    # ---- half-layers
    ou, au = rt.Table(NU, D, ctx=ctx).fill(0.0), rt.Table(NU, D, ctx=ctx).fill(0.0)
    oi, ai = rt.Table(NI, D, ctx=ctx).fill(0.0), rt.Table(NI, D, ctx=ctx).fill(0.0)
    tu, ti = timed(lambda: rt.graph_spmm(V, ou, graph.by_user, graph.user_scale, graph.item_scale, acc=au, acc_alpha=0.25),
                   lambda: rt.graph_spmm(U, oi, graph.by_item, graph.item_scale, graph.user_scale, acc=ai, acc_alpha=0.25))
    for name, t, rows in (("user", tu, NU), ("item", ti, NI)):
        nbytes = nnz * (4 * D + 8) + rows * 4 * D * 3
        t.update(bytes=nbytes, GBs=nbytes / t["ms_median"] / 1e6, of_copy_rate=nbytes / t["ms_median"] / 1e6 / copy_gbs)
        out["half_layer_" + name] = t
    out["item_over_user_per_byte"] = (ti["ms_median"] / ti["bytes"]) / (tu["ms_median"] / tu["bytes"])
    n_item = np.diff(graph.by_item.ptr)
    edges = [0, 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 2048, 8192, 32768, 131072, 1 << 30]
    out["item_row_lengths"] = dict(edges=edges[:-1], rows=[int(x) for x in np.histogram(n_item, edges)[0]], longest=int(n_item.max()),
                                   entries=[int(n_item[(n_item >= a) & (n_item < b)].sum()) for a, b in zip(edges[:-1], edges[1:])])
    # the control: the same half-layer with the items drawn uniformly -- even rows in both directions, every gathered row as far
    # away as a row of the item direction above (the user direction above gathers Zipf-popular rows, which the caches serve)
    flat = rt.InteractionGraph(records(zipf=False), NU, NI, norm="sym", ctx=ctx)
    tf, = timed(lambda: rt.graph_spmm(V, ou, flat.by_user, flat.user_scale, flat.item_scale, acc=au, acc_alpha=0.25))
    fbytes = flat.nnz * (4 * D + 8) + NU * 4 * D * 3
    tf.update(nnz=flat.nnz, bytes=fbytes, GBs=fbytes / tf["ms_median"] / 1e6, of_copy_rate=fbytes / tf["ms_median"] / 1e6 / copy_gbs)
    out["half_layer_uniform_control"] = tf
    out["item_over_uniform_per_byte"] = (ti["ms_median"] / ti["bytes"]) / (tf["ms_median"] / fbytes)
    del ou, au, oi, ai, flat

    # ---- propagate against torch.sparse.mm
    net = rt.LightGCN(U, V, graph, layers=L)
    dv = torch.device("cuda", 0)
    yard = None
    try:
        with torch.cuda.stream(stream):
            def csr_tensor(csr, rs, cs, shape):
                ptr = torch.from_numpy(csr.ptr).to(dv); cols = torch.from_numpy(csr.cols.astype(np.int64)).to(dv)
                rows = torch.repeat_interleave(torch.arange(shape[0], device=dv), ptr[1:] - ptr[:-1])
                return torch.sparse_csr_tensor(ptr, cols, rs[rows] * cs[cols], size=shape)
            A_ui = csr_tensor(graph.by_user, graph.user_scale, graph.item_scale, (NU, NI))
            A_iu = csr_tensor(graph.by_item, graph.item_scale, graph.user_scale, (NI, NU))
            Ut = torch.from_numpy(U.read()).to(dv); Vt = torch.from_numpy(V.read()).to(dv)

            def yardstick():
                cu, cv = Ut, Vt
                fu, fv = 0.25 * cu, 0.25 * cv
                for _ in range(L):
                    nu, nv = torch.sparse.mm(A_ui, cv), torch.sparse.mm(A_iu, cu)
                    fu.add_(nu, alpha=0.25); fv.add_(nv, alpha=0.25)
                    cu, cv = nu, nv
                return fu, fv
            fu, fv = yardstick()
            Uf, Vf = net.propagate(force=True)
            stream.synchronize()
            out["yardstick_max_diff"] = float(max((fu - torch.from_numpy(Uf.read()).to(dv)).abs().max(),
                                                  (fv - torch.from_numpy(Vf.read()).to(dv)).abs().max()))
        yard = yardstick
    except Exception as e:                                   # noqa: BLE001 (what torch cannot do on this box is a result)
        out["yardstick_error"] = f"{type(e).__name__}: {e}"[:300]
    if yard is not None:
        tp, ty = timed(lambda: net.propagate(force=True), yard)
        out["propagate"], out["yardstick_torch_sparse_mm"] = tp, ty
        out["propagate_over_yardstick"] = tp["ms_median"] / ty["ms_median"]
    else:
        out["propagate"], = timed(lambda: net.propagate(force=True))
    pbytes = L * (2 * nnz * (4 * D + 8) + (NU + NI) * 4 * D * 3) + (NU + NI) * 4 * D * 2
    out["propagate"].update(bytes=pbytes, of_copy_rate=pbytes / out["propagate"]["ms_median"] / 1e6 / copy_gbs)

    # ---- the step
    rng = np.random.default_rng(3)
    with torch.cuda.stream(stream):
        ids = [torch.from_numpy(rng.integers(0, n, B).astype(np.int32)).to(dv) for n in (NU, NI, NI)]
        stream.synchronize()
    for name, opt in (("sgd", rt.Optimizer.sgd(lr=0.05, ctx=ctx)), ("adam", rt.Optimizer.adam(lr=0.001, ctx=ctx))):
        out["step_" + name], = timed(lambda: net.step(opt, *ids, l2_reg=1e-4, want_loss=False))
    ctx.check_index_error()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lightgcn_bench.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(measure(args.reps, args.warmup)))
        return
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--warmup", str(args.warmup)],
                       capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit(r.returncode)
    res = json.loads(next(line for line in r.stdout.splitlines() if line.startswith("RESULT "))[7:])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for k in ("half_layer_user", "half_layer_item", "half_layer_uniform_control", "propagate", "yardstick_torch_sparse_mm", "step_sgd", "step_adam"):
        if k in res:
            print(f"{k:28s} {res[k]['ms_median']:9.3f} ms" + (f"   {res[k]['of_copy_rate']:.3f} of the copy rate" if "of_copy_rate" in res[k] else ""))
    print("item / user per byte", round(res["item_over_user_per_byte"], 3), "  item / uniform control per byte", round(res["item_over_uniform_per_byte"], 3), "  copy rate", round(res["copy_GBs"]), "GB/s")


if __name__ == "__main__":
    main()
