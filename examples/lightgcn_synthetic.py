#!/usr/bin/env python3
"""LightGCN next to BPR on a small planted-cluster set, with the same budget: the same triplets from `DeviceSampler.pairwise`, the
same optimizer, batch size and number of steps.  LightGCN scores the embeddings propagated over the user-item graph
(`LightGCN.fit_graph` -> `rt.InteractionGraph`, `train_steps` -> `rt.LightGCN.step`); BPR (without item biases) scores the raw
rows.  Users belong to clusters and like their cluster's items; a fifth of every user's items is held out, and the script prints
Recall@K of the held-out items among the items the user has not trained on, for both models.

    python examples/lightgcn_synthetic.py [--steps 300] [--dim 64] [--layers 3] [--k 20]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openrec_amd import runtime as rt                             # noqa: E402
from openrec_amd.tf2.recommenders import BPR, LightGCN            # noqa: E402


def planted(total_users=4000, total_items=3000, clusters=40, per_user=25, noise=0.15, seed=0):
    """every user draws per_user items, mostly from its cluster's share of the items"""
    rng = np.random.default_rng(seed)
    share = total_items // clusters
    rec = []
    for u in range(total_users):
        c = u % clusters
        own = c * share + rng.choice(share, per_user, replace=False)
        stray = rng.random(per_user) < noise
        own[stray] = rng.integers(0, total_items, int(stray.sum()))
        rec += [(u, int(i)) for i in np.unique(own)]
    rec = np.array(rec, dtype=[("user_id", np.int32), ("item_id", np.int32)])
    rng.shuffle(rec)
    return rec, total_users, total_items


def recall_at(model, users, excl, held, k):
    items, _ = model.recommend(users, k, excl)
    hits = sum(len(set(row.tolist()) & held[int(u)]) for u, row in zip(users, np.asarray(items)))
    return hits / sum(min(k, len(held[int(u)])) for u in users)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--k", type=int, default=20)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    raw, NU, NI = planted()
    test = np.arange(raw.size) % 5 == 0
    train, heldout = raw[~test], raw[test]
    users = np.arange(0, NU, 4, dtype=np.int32)
    held = {int(u): set() for u in users}
    for u, i in zip(heldout["user_id"], heldout["item_id"]):
        if int(u) in held:
            held[int(u)].add(int(i))
    data = rt.ALSData(train, NU, NI)                                  # both CSRs, built once, kept on the device
    excl = rt.SparseMask.from_lists([data.by_user.cols[data.by_user.ptr[u]:data.by_user.ptr[u + 1]] for u in users], NI)
    sampler = rt.DeviceSampler(train, NU, NI)
    uid, pid, nid = (torch.empty(args.batch, dtype=torch.int32, device=dev) for _ in range(3))

    gcn = LightGCN(args.dim, NU, NI, layers=args.layers, l2_reg=1e-4).fit_graph(data)
    bpr = BPR(args.dim, args.dim, NU, NI, use_item_bias=False, l2_reg=1e-4)
    opt_g, opt_b = rt.Optimizer.adam(0.005), rt.Optimizer.adam(0.005)
    print(f"{data.nnz} observations, {NU} x {NI}, D = {args.dim}, L = {args.layers}, B = {args.batch}, Adam(0.005)")
    print(f"  start     : recall@{args.k}  LightGCN {recall_at(gcn, users, excl, held, args.k):.4f}   BPR {recall_at(bpr, users, excl, held, args.k):.4f}")
    for step in range(args.steps):
        sampler.pairwise(1, step * args.batch, args.batch, uid, pid, nid)
        gcn.train_steps(opt_g, uid, pid, nid, K=1, want_loss=False)
        bpr.train_steps(opt_b, uid, pid, nid, K=1, want_loss=False)
        if (step + 1) % 100 == 0 or step + 1 == args.steps:
            print(f"  step {step + 1:5d}: recall@{args.k}  LightGCN {recall_at(gcn, users, excl, held, args.k):.4f}   "
                  f"BPR {recall_at(bpr, users, excl, held, args.k):.4f}")


if __name__ == "__main__":
    main()
