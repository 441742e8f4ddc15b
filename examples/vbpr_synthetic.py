#!/usr/bin/env python3
"""VBPR next to BPR on items nobody has interacted with yet, with the same budget: the same triplets from `DeviceSampler.pairwise`,
the same optimizer, batch size and number of steps.  Every item has a hidden taste vector and a feature row made from it by a
planted low-rank map plus noise; users like the items whose taste is near their own.  A tenth of the items is HELD OUT: none of their
interactions is trained on.  BPR knows an item by its id alone, so a held-out item keeps its initial vector; VBPR scores it through
F[i] E, learned on the other items.  The script prints Recall@K on the held-out items, ranked among themselves, for both models.

    python examples/vbpr_synthetic.py [--steps 400] [--k 20]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openrec_amd import runtime as rt                             # noqa: E402
from openrec_amd.tf2.recommenders import BPR, VBPR                # noqa: E402


def planted(total_users=4000, total_items=3000, rank=8, feature_dim=64, per_user=40, noise=0.1, seed=0):
    """-> interactions, item features [items, feature_dim]; a user's items are its per_user best by taste among a random half"""
    rng = np.random.default_rng(seed)
    taste_u = rng.standard_normal((total_users, rank)); taste_i = rng.standard_normal((total_items, rank))
    F = taste_i @ rng.standard_normal((rank, feature_dim)) / np.sqrt(rank) + noise * rng.standard_normal((total_items, feature_dim))
    rec = []
    for u in range(total_users):
        seen = rng.choice(total_items, total_items // 2, replace=False)
        best = seen[np.argsort(-(taste_i[seen] @ taste_u[u]))[:per_user]]
        rec += [(u, int(i)) for i in best]
    rec = np.array(rec, dtype=[("user_id", np.int32), ("item_id", np.int32)])
    rng.shuffle(rec)
    return rec, F.astype(np.float32), total_users, total_items


def recall_at(model, users, excl, held, k):
    items, _ = model.recommend(users, k, excl)
    hits = sum(len(set(row.tolist()) & held[int(u)]) for u, row in zip(users, np.asarray(items)))
    return hits / max(1, sum(min(k, len(held[int(u)])) for u in users))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--k", type=int, default=20)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    raw, F, NU, NI = planted()
    cold = np.arange(NI) % 10 == 0                                     # the held-out items
    is_cold = cold[raw["item_id"]]
    train, heldout = raw[~is_cold], raw[is_cold]
    users = np.arange(0, NU, 4, dtype=np.int32)
    held = {int(u): set() for u in users}
    for u, i in zip(heldout["user_id"], heldout["item_id"]):
        if int(u) in held:
            held[int(u)].add(int(i))
    warm = np.flatnonzero(~cold)
    excl = rt.SparseMask.from_lists([warm for _ in users], NI)        # rank the held-out items among themselves
    sampler = rt.DeviceSampler(train, NU, NI)
    uid, pid, nid = (torch.empty(args.batch, dtype=torch.int32, device=dev) for _ in range(3))

    Dl, Dc = 32, 32
    vbpr = VBPR(Dl + Dc, Dl, NU, NI, item_features=F, l2_reg=1e-4, l2_reg_mlp=1e-4)
    bpr = BPR(Dl + Dc, Dl + Dc, NU, NI, l2_reg=1e-4)
    opt_v, opt_b = rt.Optimizer.adam(0.005), rt.Optimizer.adam(0.005)
    print(f"{train.size} training interactions, {NU} x {NI}, {int(cold.sum())} held-out items with {heldout.size} interactions, "
          f"Fd = {F.shape[1]}, Dl = Dc = 32, B = {args.batch}, Adam(0.005)")
    print(f"  start     : recall@{args.k} on the held-out items  VBPR {recall_at(vbpr, users, excl, held, args.k):.4f}   "
          f"BPR {recall_at(bpr, users, excl, held, args.k):.4f}")
    for step in range(args.steps):
        sampler.pairwise(1, step * args.batch, args.batch, uid, pid, nid)
        vbpr.train_steps(opt_v, uid, pid, nid, K=1, want_loss=False)
        bpr.train_steps(opt_b, uid, pid, nid, K=1, want_loss=False)
        if (step + 1) % 100 == 0 or step + 1 == args.steps:
            print(f"  step {step + 1:5d}: recall@{args.k} on the held-out items  VBPR {recall_at(vbpr, users, excl, held, args.k):.4f}   "
                  f"BPR {recall_at(bpr, users, excl, held, args.k):.4f}")


if __name__ == "__main__":
    main()
