#!/usr/bin/env python3
"""BPR's tables under a sampled-softmax loss, entirely on the device: sampler -> N-negative train step -> sampler, ids never
leave HBM.  Two runs on the same synthetic interactions (a planted low-rank preference model) and the same positives: BPR on
one uniform negative per positive (`DeviceSampler.pairwise` + `rt.pairwise_step`) and sampled softmax on 16
(`DeviceSampler.pairwise_multi` + `rt.multineg_step`).  Both print the BPR loss on a fixed uniform probe batch -- one yardstick
for both objectives -- and recall@20 of the probe users' training positives among all items.

    python examples/bpr_sampled_softmax.py [--steps 300] [--negatives 16]
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


def recall_at(U, V, b, users, positives, k=20):
    """the share of the users' positives among their k best items"""
    items, _ = rt.recommend_topk("dot", U, V, b, users, k)
    hits = sum(len(set(row.tolist()) & positives[u]) for u, row in zip(users, np.asarray(items)))
    return hits / sum(min(k, len(positives[u])) for u in users)


def train(sampler, NU, NI, steps, B, negatives, probe, users, positives, log):
    import torch
    dev = torch.device("cuda", 0)
    U = rt.Table(NU, 64).init_uniform(seed=1); V = rt.Table(NI, 64).init_uniform(seed=2); b = rt.Table(NI, 1).fill(0.0)
    opt = rt.Optimizer.adagrad(0.1)
    uid, pid = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))
    nid = torch.empty((B, max(negatives, 1)), dtype=torch.int32, device=dev)
    for step in range(steps):
        want = (step + 1) % log == 0
        if negatives > 1:
            sampler.pairwise_multi(1, step * B, B, uid, pid, nid, negatives=negatives)
            out = rt.multineg_step("softmax", opt, U, V, b, uid, pid, nid, K=1, B=B, l2_reg=0.01, want_loss=want)     # same stream, no sync
        else:
            sampler.pairwise(1, step * B, B, uid, pid, nid)
            out = rt.pairwise_step("bpr", opt, U, V, b, uid, pid, nid.reshape(-1), K=1, B=B, l2_reg=0.01, want_loss=want)
        if want:
            probe_loss, _ = rt.pairwise_loss("bpr", U, V, b, *probe)
            print(f"  step {step + 1:4d}  train loss {out[0][0]:.4f}  BPR loss on the uniform probe batch {probe_loss:.4f}  "
                  f"recall@20 {recall_at(U, V, b, users, positives):.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--negatives", type=int, default=16)
    args = ap.parse_args()
    import torch
    raw, NU, NI = synthetic()
    sampler = rt.DeviceSampler(raw, NU, NI)
    dev = torch.device("cuda", 0)
    probe = [torch.empty(8192, dtype=torch.int32, device=dev) for _ in range(3)]
    sampler.pairwise(99, 0, 8192, *probe)
    users = np.arange(0, NU, 8, dtype=np.int32)
    positives = {int(u): set() for u in users}
    for u, i in zip(raw["user_id"], raw["item_id"]):
        if int(u) in positives:
            positives[int(u)].add(int(i))
    for name, n in (("BPR, one uniform negative", 1), (f"sampled softmax, {args.negatives} uniform negatives", args.negatives)):
        print(name)
        train(sampler, NU, NI, args.steps, args.batch, n, probe, users, positives, max(1, args.steps // 6))


if __name__ == "__main__":
    main()
