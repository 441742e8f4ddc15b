#!/usr/bin/env python3
"""BPR with popularity-weighted negatives, entirely on the device: `DeviceSampler.set_proposal(popularity=0.75)` makes the
sampler draw every negative in proportion to (distinct users of the item) ** 0.75 -- the word2vec proposal -- instead of
uniformly over the catalogue; sampler -> fused train step -> sampler, ids never leave HBM.  Three runs on the same synthetic
interactions (a planted low-rank preference model whose items follow a Zipf law) and the same positives: uniform negatives,
popularity negatives, and the hardest of M popularity-drawn candidates (`pairwise_hard` draws its candidates from the proposal
too).  Under a Zipf law a uniform negative is nearly always an item from the long tail, which the model learns to push down at
once; popular items, the ones a recommender must rank among, come up as negatives only with the proposal.  The loss on a fixed
popularity-weighted probe batch shows what each run has learned about them.

    python examples/bpr_popularity_negatives.py [--steps 300] [--candidates 8] [--alpha 0.75]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openrec_amd import runtime as rt                             # noqa: E402


def synthetic(total_users=4000, total_items=6000, per_user=30, rank=8, zipf=1.05, seed=0):
    rng = np.random.default_rng(seed)
    pu, qi = rng.normal(size=(total_users, rank)), rng.normal(size=(total_items, rank))
    law = 1.0 / np.arange(1, total_items + 1) ** zipf
    law /= law.sum()
    rec = []
    for u in range(total_users):
        cand = rng.choice(total_items, 300, replace=False, p=law)          # what the user gets to see follows the Zipf law
        rec += [(u, i) for i in cand[np.argsort(-(qi[cand] @ pu[u]))[:per_user]]]
    rec = np.array(rec, dtype=[("user_id", np.int32), ("item_id", np.int32)])
    rng.shuffle(rec)
    return rec, total_users, total_items


def train(sampler, NU, NI, steps, B, candidates, probe, log):
    import torch
    dev = torch.device("cuda", 0)
    U = rt.Table(NU, 64).init_uniform(seed=1); V = rt.Table(NI, 64).init_uniform(seed=2); b = rt.Table(NI, 1).fill(0.0)
    opt = rt.Optimizer.adagrad(0.1)
    uid, pid, nid = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    for step in range(steps):
        if candidates > 1:
            sampler.pairwise_hard(1, step * B, B, uid, pid, nid, "bpr", U, V, b, candidates=candidates)
        else:
            sampler.pairwise(1, step * B, B, uid, pid, nid)
        want = (step + 1) % log == 0
        out = rt.pairwise_step("bpr", opt, U, V, b, uid, pid, nid, K=1, B=B, want_loss=want)     # same stream, no sync
        if want:
            probe_loss, _ = rt.pairwise_loss("bpr", U, V, b, *probe)
            print(f"  step {step + 1:4d}  train loss {out[0][0]:.4f}  loss on the popularity-weighted probe batch {probe_loss:.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--alpha", type=float, default=0.75)
    args = ap.parse_args()
    import torch
    raw, NU, NI = synthetic()
    sampler = rt.DeviceSampler(raw, NU, NI)
    dev = torch.device("cuda", 0)
    probe = [torch.empty(8192, dtype=torch.int32, device=dev) for _ in range(3)]
    sampler.set_proposal(popularity=args.alpha)
    sampler.pairwise(99, 0, 8192, *probe)
    runs = (("uniform negatives", None, 1), (f"negatives ~ popularity^{args.alpha:g}", args.alpha, 1),
            (f"hardest of {args.candidates} candidates ~ popularity^{args.alpha:g}", args.alpha, args.candidates))
    for name, alpha, m in runs:
        print(name)
        sampler.set_proposal(popularity=alpha)                    # None: uniform again
        train(sampler, NU, NI, args.steps, args.batch, m, probe, max(1, args.steps // 6))


if __name__ == "__main__":
    main()
