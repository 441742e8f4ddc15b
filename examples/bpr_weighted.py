#!/usr/bin/env python3
"""BPR with recency-weighted interactions and an l2 coefficient, entirely on the device.  Synthetic interactions carry a
timestamp; the preference model they were drawn from drifts over time, so old interactions describe a user who no longer exists.
Every record gets the weight exp(-age / tau); `DeviceSampler.set_record_weights` keeps the weights in HBM, and the loop is
sampler -> `pairwise_weights` -> `rt.pairwise_step(weights=..., l2_reg=0.01)`: ids and weights never leave the device, and the
objective is mean_i w_i * (-log sigmoid x_i) + 0.01 * l2_loss.  Two runs on the same positives and negatives, unweighted and
weighted, and their loss on a probe batch of the most recent interactions.

    python examples/bpr_weighted.py [--steps 300] [--tau 0.2] [--l2-reg 0.01]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openrec_amd import runtime as rt                             # noqa: E402


def synthetic(total_users=4000, total_items=6000, per_user=30, rank=8, seed=0):
    """(records, timestamps in [0, 1]): a user's taste moves from one random vector to another as time passes"""
    rng = np.random.default_rng(seed)
    p0, p1, qi = rng.normal(size=(total_users, rank)), rng.normal(size=(total_users, rank)), rng.normal(size=(total_items, rank))
    rec, ts = [], []
    for u in range(total_users):
        t = np.sort(rng.random(per_user))
        for tt in t:
            cand = rng.integers(0, total_items, 40)
            rec.append((u, cand[np.argmax(qi[cand] @ ((1 - tt) * p0[u] + tt * p1[u]))])); ts.append(tt)
    rec = np.array(rec, dtype=[("user_id", np.int32), ("item_id", np.int32)])
    order = rng.permutation(len(rec))
    return rec[order], np.array(ts)[order], total_users, total_items


def train(sampler, NU, NI, steps, B, weighted, l2_reg, probe, log):
    import torch
    dev = torch.device("cuda", 0)
    U = rt.Table(NU, 64).init_uniform(seed=1); V = rt.Table(NI, 64).init_uniform(seed=2); b = rt.Table(NI, 1).fill(0.0)
    opt = rt.Optimizer.adagrad(0.1)
    uid, pid, nid = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    w = torch.empty(B, dtype=torch.float32, device=dev)
    for step in range(steps):
        sampler.pairwise(1, step * B, B, uid, pid, nid)
        if weighted:
            sampler.pairwise_weights(1, step * B, B, w)           # the weight of the record each sample drew, same stream
        want = (step + 1) % log == 0
        out = rt.pairwise_step("bpr", opt, U, V, b, uid, pid, nid, K=1, B=B, want_loss=want, weights=w if weighted else None, l2_reg=l2_reg)
        if want:
            probe_loss, _ = rt.pairwise_loss("bpr", U, V, b, *probe)
            print(f"  step {step + 1:4d}  train loss {out[0][0]:.4f}  l2_loss {out[1][0]:.1f}  loss on the recent interactions {probe_loss:.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--tau", type=float, default=0.2)
    ap.add_argument("--l2-reg", type=float, default=0.01)
    args = ap.parse_args()
    import torch
    raw, ts, NU, NI = synthetic()
    sampler = rt.Sampler(raw, NU, NI)
    sampler.set_record_weights(np.exp(-(ts.max() - ts) / args.tau))
    # the probe: the most recent tenth of the interactions as positives, uniform negatives
    recent = raw[ts >= np.quantile(ts, 0.9)][:8192]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    probe = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev)
             for x in (recent["user_id"], recent["item_id"], rng.integers(0, NI, len(recent)))]
    for name, weighted in (("every interaction counts the same", False), (f"weights exp(-age / {args.tau:g})", True)):
        print(f"{name}, l2_reg = {args.l2_reg:g}")
        train(sampler, NU, NI, args.steps, args.batch, weighted, args.l2_reg, probe, max(1, args.steps // 6))


if __name__ == "__main__":
    main()
