#!/usr/bin/env python3
"""BPR trained with WARP negatives, entirely on the device: `DeviceSampler.pairwise_warp` draws candidates for every triplet until
one scores above the positive (margin 0), hands the fused step that first violator and, as the triplet's weight, the rank loss
log(floor((items - 1) / trials)); `rt.pairwise_step(..., weights=w, l2_reg=...)` trains on them on the same stream -- ids and
weights never leave HBM and nothing synchronises in between.  A triplet without a violator among `--trials` candidates has weight
0 and keeps only its l2 part.  Per epoch: the mean number of trials of the triplets that found a violator and the share of
triplets without one -- both rise as the model learns to rank the positives first -- and the loss on a fixed uniform probe batch.

    python examples/bpr_warp.py [--epochs 6] [--trials 16]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openrec_amd import runtime as rt                             # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--trials", type=int, default=16)
    ap.add_argument("--l2", type=float, default=1e-5)
    args = ap.parse_args()
    import torch
    raw, NU, NI = synthetic()
    sampler = rt.DeviceSampler(raw, NU, NI)
    dev = torch.device("cuda", 0)
    B, T = args.batch, args.trials
    probe = [torch.empty(8192, dtype=torch.int32, device=dev) for _ in range(3)]
    sampler.pairwise(99, 0, 8192, *probe)
    U = rt.Table(NU, 64).init_uniform(seed=1); V = rt.Table(NI, 64).init_uniform(seed=2); b = rt.Table(NI, 1).fill(0.0)
    opt = rt.Optimizer.adam(0.02)          # (lazily applied: the sampler brings the tables up to date before it gathers)
    table = rt.warp_weights(NI, T, "log", normalize=True)         # the same array every call: no upload, no synchronisation
    steps = len(raw) // B
    uid, pid, nid = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    w = torch.empty(B, dtype=torch.float32, device=dev)
    trials = torch.empty(steps * B, dtype=torch.int32, device=dev)        # an epoch's trial counts, read once per epoch
    for epoch in range(args.epochs):
        for step in range(steps):
            g = (epoch * steps + step) * B
            sampler.pairwise_warp(1, g, B, uid, pid, nid, w, "bpr", U, V, b, max_trials=T, margin=0.0, rank_weight=table,
                                  trials_out=trials[step * B:(step + 1) * B])
            rt.pairwise_step("bpr", opt, U, V, b, uid, pid, nid, K=1, B=B, weights=w, l2_reg=args.l2, want_loss=False)
        sampler.ctx.synchronize()
        t = trials.cpu().numpy()
        found = t > 0
        probe_loss, _ = rt.pairwise_loss("bpr", U, V, b, *probe)
        print(f"epoch {epoch + 1}: mean trials {t[found].mean() if found.any() else 0.0:5.2f}   without a violator "
              f"{100.0 * (~found).mean():5.1f} %   loss on the uniform probe batch {probe_loss:.4f}")


if __name__ == "__main__":
    main()
