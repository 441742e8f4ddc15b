#!/usr/bin/env python3
"""BPR's tables trained on in-batch negatives, entirely on the device: `DeviceSampler.pairwise` draws (user, positive) pairs --
its negative is not used --, and `rt.inbatch_step` scores every positive against the positives of the whole batch under a
softmax with the log-Q correction: an item that is popular shows up as an in-batch negative in proportion to its count, so
-log Q(item) is added to its column (Yi et al. 2019).  The counts are taken from the interactions with NumPy once.  The run
prints the train loss and recall@20 of some users' training positives among all items (`rt.recommend_topk`), with and without
the correction.

    python examples/bpr_inbatch.py [--steps 300] [--batch 4096] [--temperature 0.5]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openrec_amd import runtime as rt                             # noqa: E402


def synthetic(total_users=4000, total_items=6000, per_user=30, rank=8, seed=0):
    """a planted low-rank preference model with a popularity skew: a user's candidates are drawn with Zipf-like weights"""
    rng = np.random.default_rng(seed)
    pu, qi = rng.normal(size=(total_users, rank)), rng.normal(size=(total_items, rank))
    pop = 1.0 / np.arange(1, total_items + 1) ** 0.7
    pop /= pop.sum()
    rec = []
    for u in range(total_users):
        cand = rng.choice(total_items, 300, replace=False, p=pop)
        rec += [(u, i) for i in cand[np.argsort(-(qi[cand] @ pu[u]))[:per_user]]]
    rec = np.array(rec, dtype=[("user_id", np.int32), ("item_id", np.int32)])
    rng.shuffle(rec)
    return rec, total_users, total_items


def recall_at(U, V, b, users, positives, k=20):
    """the share of the users' positives among their k best items"""
    items, _ = rt.recommend_topk("dot", U, V, b, users, k)
    hits = sum(len(set(row.tolist()) & positives[u]) for u, row in zip(users, np.asarray(items)))
    return hits / sum(min(k, len(positives[u])) for u in users)


def train(sampler, NU, NI, steps, B, scale, neg_log_q, users, positives, log):
    import torch
    dev = torch.device("cuda", 0)
    U = rt.Table(NU, 64).init_uniform(seed=1); V = rt.Table(NI, 64).init_uniform(seed=2)
    opt = rt.Optimizer.adam(0.01)                                     # (the loss is a mean over B: Adam does not care about the 1 / B)
    uid, pid, unused = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    for step in range(steps):
        want = (step + 1) % log == 0
        sampler.pairwise(1, step * B, B, uid, pid, unused)
        sampler.ctx.synchronize()                                     # (the gather below runs on torch's stream)
        off = neg_log_q[pid.long()].contiguous() if neg_log_q is not None else None
        out = rt.inbatch_step(opt, U, V, None, uid, pid, K=1, B=B, item_offset=off, scale=scale, l2_reg=1e-6, want_loss=want)
        if want:
            print(f"  step {step + 1:4d}  train loss {out[0][0]:.4f}  recall@20 {recall_at(U, V, None, users, positives):.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--temperature", type=float, default=0.5)
    args = ap.parse_args()
    import torch
    raw, NU, NI = synthetic()
    sampler = rt.DeviceSampler(raw, NU, NI)
    counts = np.bincount(raw["item_id"], minlength=NI).astype(np.float64)
    q = np.maximum(counts, 0.5) / counts.sum()                        # the in-batch sampling probability of an item
    neg_log_q = torch.from_numpy((-np.log(q)).astype(np.float32)).cuda()
    users = np.arange(0, NU, 8, dtype=np.int32)
    positives = {int(u): set() for u in users}
    for u, i in zip(raw["user_id"], raw["item_id"]):
        if int(u) in positives:
            positives[int(u)].add(int(i))
    for name, off in (("in-batch softmax, no correction", None), ("in-batch softmax with the log-Q correction", neg_log_q)):
        print(name)
        train(sampler, NU, NI, args.steps, args.batch, 1.0 / args.temperature, off, users, positives, max(1, args.steps // 6))


if __name__ == "__main__":
    main()
