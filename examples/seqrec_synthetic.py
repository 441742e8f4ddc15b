#!/usr/bin/env python3
"""A recommender without a user table on sequences with planted next-item structure.  Items fall into groups; a user's next item
comes from the group that FOLLOWS the group of the item before it (with probability 0.85, else from anywhere), so the last few
items of a history say where the next one lies and who the user is says nothing.  VanillaYouTubeRec pools the history's item
embeddings into the user vector and is trained on one half of the users; it then recommends for the OTHER half from their
histories alone -- no step is ever taken on them.  The script prints Recall@K of the held-out users' last item beside a
popularity baseline (the K most frequent items of the training half).

    python examples/seqrec_synthetic.py [--steps 600] [--k 20]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openrec_amd import runtime as rt                                     # noqa: E402
from openrec_amd.tf2 import data                                          # noqa: E402
from openrec_amd.tf2.recommenders import VanillaYouTubeRec                # noqa: E402


def planted(total_users=6000, total_items=2000, groups=50, length=30, follow=0.85, seed=0):
    """-> records in time order per user ('user_id', 'item_id', 'ts')"""
    rng = np.random.default_rng(seed)
    per = total_items // groups
    skew = 1.0 / np.arange(1, per + 1) ** 0.5                       # mild popularity inside a group
    skew /= skew.sum()
    cur = rng.integers(0, total_items, total_users)
    cols = [cur]
    for _ in range(length - 1):
        g = (cur // per + 1) % groups
        nxt = g * per + rng.choice(per, total_users, p=skew)
        jump = rng.random(total_users) >= follow
        nxt[jump] = rng.integers(0, total_items, int(jump.sum()))
        cols.append(nxt)
        cur = nxt
    seqs = np.stack(cols, 1)
    rec = np.zeros(total_users * length, dtype=[("user_id", np.int32), ("item_id", np.int32), ("ts", np.int64)])
    rec["user_id"] = np.repeat(np.arange(total_users), length)
    rec["item_id"] = seqs.reshape(-1)
    rec["ts"] = np.tile(np.arange(length), total_users)
    rng.shuffle(rec)                                                # the generators order a user's records by `ts`
    return rec, total_users, total_items


def recall_at(model, ev, k):
    items, _ = model.recommend(ev["seq_item_id"], ev["seq_len"], k)
    return float((np.asarray(items) == ev["label"][:, None]).any(1).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--negatives", type=int, default=16)
    ap.add_argument("--seq", type=int, default=5)
    ap.add_argument("--k", type=int, default=20)
    args = ap.parse_args()
    raw, NU, NI = planted()
    train_half = raw["user_id"] % 2 == 0
    train, held = raw[train_half], raw[~train_half]
    ev = next(data.temporal_evaluation(held, NU, args.seq, time_field="ts"))
    pop = np.argsort(-np.bincount(train["item_id"], minlength=NI), kind="stable")[:args.k]
    pop_recall = float(np.isin(ev["label"], pop).mean())

    model = VanillaYouTubeRec(dim_item_embed=32, max_seq_len=args.seq, total_items=NI, l2_reg_embed=1e-5, pool="mean")
    opt = rt.Optimizer.adam(0.01)
    rng = np.random.default_rng(1)
    print(f"{train.size} training records of {NU // 2} users, {len(ev['label'])} held-out users, {NI} items, histories of up to {args.seq}, "
          f"D = 32, B = {args.batch}, N = {args.negatives}, sampled softmax, Adam(0.01)")
    print(f"  popularity baseline: recall@{args.k} {pop_recall:.4f}")
    print(f"  start     : recall@{args.k} for the held-out users {recall_at(model, ev, args.k):.4f}")
    batches = data.temporal_batches(train, NU, args.batch, args.seq, seed=2, time_field="ts")
    for step in range(args.steps):
        bt = next(batches)
        nid = rng.integers(0, NI, (args.batch, args.negatives)).astype(np.int32)
        loss = model.train_steps(opt, bt["seq_item_id"], bt["seq_len"], bt["label"], nid, loss="softmax", want_loss=(step + 1) % 100 == 0)
        if (step + 1) % 100 == 0 or step + 1 == args.steps:
            tail = f"loss {loss[0][0]:.4f}  " if loss is not None else ""
            print(f"  step {step + 1:5d}: {tail}recall@{args.k} for the held-out users {recall_at(model, ev, args.k):.4f}")


if __name__ == "__main__":
    main()
