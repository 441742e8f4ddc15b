#!/usr/bin/env python3
"""WRMF trained by alternating least squares on the device (`WRMF.fit_als` -> `rt.als_sweep`): no sampler, no learning rate, every
row solved in closed form over ALL user x item cells.  Synthetic interactions from a planted low-rank preference model; a fifth
of every user's items is held out, and after each sweep the script prints recall@20 of the held-out items among the items the
user has not trained on and the objective the sweeps descend (`WRMF.als_objective`, computed on the device) -- next to the
recall of WRMF trained the reference's way, by SGD over sampled points.  `--solver cg` takes `--cg-steps` conjugate-gradient
steps per row from its current value instead of the closed form.

    python examples/wrmf_als.py [--sweeps 5] [--dim 64] [--solver cholesky|cg] [--cg-steps 3]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openrec_amd import runtime as rt                             # noqa: E402
from openrec_amd.tf2.recommenders import WRMF                     # noqa: E402


def synthetic(total_users=4000, total_items=6000, per_user=30, rank=8, seed=0):
    rng = np.random.default_rng(seed)
    pu, qi = rng.normal(size=(total_users, rank)), rng.normal(size=(total_items, rank))
    rec = []
    for u in range(total_users):
        cand = rng.choice(total_items, 300, replace=False)
        rec += [(u, i) for i in cand[np.argsort(-(qi[cand] @ pu[u]))[:per_user]]]
    rec = np.array(rec, dtype=[("user_id", np.int32), ("item_id", np.int32)])
    rng.shuffle(rec)
    return rec, total_users, total_items


def recall_at(model, users, excl, held, k=20):
    items, _ = model.recommend(users, k, excl)
    hits = sum(len(set(row.tolist()) & held[int(u)]) for u, row in zip(users, np.asarray(items)))
    return hits / sum(min(k, len(held[int(u)])) for u in users)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=5)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--reg", type=float, default=1.0)
    ap.add_argument("--solver", choices=("cholesky", "cg"), default="cholesky")
    ap.add_argument("--cg-steps", type=int, default=3)
    args = ap.parse_args()
    raw, NU, NI = synthetic()
    test = np.arange(raw.size) % 5 == 0
    train, heldout = raw[~test], raw[test]
    users = np.arange(0, NU, 4, dtype=np.int32)
    held = {int(u): set() for u in users}
    for u, i in zip(heldout["user_id"], heldout["item_id"]):
        if int(u) in held:
            held[int(u)].add(int(i))
    data = rt.ALSData(train, NU, NI)                                  # both CSRs, built once, kept on the device
    excl = rt.SparseMask.from_lists([data.by_user.cols[data.by_user.ptr[u]:data.by_user.ptr[u + 1]] for u in users], NI)

    model = WRMF(args.dim, args.dim, NU, NI, a=10.0, b=1.0)
    model.item_bias.table.fill(0.0)                                   # ALS has no bias term
    how = "Cholesky" if args.solver == "cholesky" else f"{args.cg_steps} CG steps per row"
    print(f"ALS ({how}): {data.nnz} observations, {NU} x {NI}, D = {args.dim}, a = 10, b = 1, reg = {args.reg}")
    print(f"  start  : objective {model.als_objective(data, reg=args.reg):.6g}")
    for sweep in range(args.sweeps):
        t0 = time.perf_counter()
        model.fit_als(data, sweeps=1, reg=args.reg, solver=args.solver, cg_steps=args.cg_steps)
        rt.default_context().synchronize()
        dt = time.perf_counter() - t0
        print(f"  sweep {sweep + 1}: {dt * 1e3:7.1f} ms   recall@20 of the held-out items {recall_at(model, users, excl, held):.4f}"
              f"   objective {model.als_objective(data, reg=args.reg):.6g}")

    # the reference's trainer for the same model: SGD over sampled (user, item, label) points
    import torch
    dev = torch.device("cuda", 0)
    sgd = WRMF(args.dim, args.dim, NU, NI, a=10.0, b=1.0)
    sgd.item_bias.table.fill(0.0)
    U, V, b = sgd._tables()
    sampler = rt.DeviceSampler(train, NU, NI)
    opt = rt.Optimizer.adagrad(0.05)
    B, steps = 8192, 600
    uid, iid = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))
    lab = torch.empty(B, dtype=torch.float32, device=dev)
    print(f"SGD over sampled points (Adagrad, B = {B}, half of each batch positives):")
    for step in range(steps):
        sampler.stratified_pointwise(1, step * B, B, 0.5, uid, iid, lab)
        rt.pointwise_step("wrmf", opt, U, V, b, None, uid, iid, lab, K=1, B=B, a=10.0, b_w=1.0, l2_reg=0.01, want_loss=False)
        if (step + 1) % 200 == 0:
            print(f"  step {step + 1:4d}: recall@20 of the held-out items {recall_at(sgd, users, excl, held):.4f}")


if __name__ == "__main__":
    main()
