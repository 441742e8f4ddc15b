#!/usr/bin/env python3
"""Mult-DAE on synthetic data with planted taste groups: every user likes two of 40 item groups and has 10 .. 40 items, most of them
from those groups.  `MultDAE.train_steps` trains on (input bag with dropped entries, the user's whole item set) under the
multinomial likelihood over ALL items -- one walk of the item table per step, whatever the sets' sizes.  Beside it, from the same
start and on the same batches, `rt.SeqRec.step_full` with ONE label per sample (a random item of the same set): the route that
was there before label sets.  Both train on one half of the users and recommend for the OTHER half from 80 % of each user's items
(the fold-in history, excluded from the answer); the script prints Recall@K of the held-out 20 % for both and, with --out, records
the numbers.  Nothing is asserted.

    python examples/multdae_synthetic.py [--steps 300] [--k 20] [--out profiles/multdae_synthetic.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openrec_amd import runtime as rt                                     # noqa: E402
from openrec_amd.tf2 import data                                          # noqa: E402
from openrec_amd.tf2.recommenders import MultDAE                          # noqa: E402


def planted(total_users=8000, total_items=2000, groups=40, seed=0):
    """-> records ('user_id', 'item_id'), every (user, item) once"""
    rng = np.random.default_rng(seed)
    per = total_items // groups
    users, items = [], []
    for u in range(total_users):
        g = rng.choice(groups, 2, replace=False)
        n = int(rng.integers(10, 41))
        own = (g[rng.integers(0, 2, n)] * per + rng.integers(0, per, n))
        noise = rng.random(n) < 0.15
        own[noise] = rng.integers(0, total_items, int(noise.sum()))
        own = np.unique(own)
        rng.shuffle(own)
        users.append(np.full(len(own), u)); items.append(own)
    rec = np.zeros(sum(len(x) for x in items), dtype=[("user_id", np.int32), ("item_id", np.int32)])
    rec["user_id"] = np.concatenate(users); rec["item_id"] = np.concatenate(items)
    return rec, total_users, total_items


def recall_at(model, ev, k, total_items):
    excl = np.zeros((len(ev["user_id"]), total_items), bool)
    rows = np.repeat(np.arange(len(ev["user_id"])), ev["excl_len"])
    live = np.arange(ev["excl_item_id"].shape[1])[None, :] < ev["excl_len"][:, None]
    excl[rows, ev["excl_item_id"][live]] = True
    got, _ = model.recommend(ev["seq_item_id"], ev["seq_len"], k, excl_mask=excl)
    got = np.asarray(got)
    hits = np.zeros(len(got))
    for i in range(len(got)):
        pos = ev["pos_item_id"][i, :ev["pos_len"][i]]
        hits[i] = np.isin(pos, got[i]).sum() / min(k, len(pos))
    return float(hits.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    raw, NU, NI = planted()
    train = raw[raw["user_id"] % 2 == 0]
    held = raw[raw["user_id"] % 2 == 1]
    rng = np.random.default_rng(5)
    fold = rng.random(held.size) < 0.8
    ev = next(data.autoencoder_evaluation(held[fold], held[~fold], NU))
    pop = np.argsort(-np.bincount(train["item_id"], minlength=NI), kind="stable")

    def model():
        return MultDAE(dim_embed=64, total_items=NI, l2_reg_embed=1e-5, pool="mean")
    sets, single = model(), model()
    for a, c in zip(sets._factors(), single._factors()):                  # the same start
        c.table.write(a.table.read())
    o_sets, o_single = rt.Optimizer.adam(0.005), rt.Optimizer.adam(0.005)
    print(f"{train.size} training records of {NU // 2} users, {len(ev['user_id'])} held-out users folded in from 80 % of their items, "
          f"{NI} items, D = 64, B = {args.batch}, Adam(0.005), input dropout 0.5")
    start = recall_at(sets, ev, args.k, NI)
    print(f"  start     : recall@{args.k} of the held-out items {start:.4f}")
    batches = data.autoencoder_batches(train, NU, args.batch, seed=2, dropout=0.5)
    t_sets = t_single = 0.0
    curve = []
    for step in range(args.steps):
        bt = next(batches)
        pick = (rng.random(args.batch) * bt["label_len"]).astype(np.int64)
        one = bt["label_items"][np.arange(args.batch), pick]
        want = (step + 1) % 100 == 0 or step + 1 == args.steps
        t0 = time.perf_counter()
        ls = sets.train_steps(o_sets, bt["in_items"], bt["in_len"], bt["label_items"], bt["label_len"], want_loss=want)
        sets._net.ctx.synchronize(); t1 = time.perf_counter()
        l1 = single.train_steps_full(o_single, bt["in_items"], bt["in_len"], one, want_loss=want)
        single._net.ctx.synchronize(); t2 = time.perf_counter()
        t_sets += t1 - t0; t_single += t2 - t1
        if want:
            r_sets, r_single = recall_at(sets, ev, args.k, NI), recall_at(single, ev, args.k, NI)
            curve.append(dict(step=step + 1, recall_sets=r_sets, recall_single_label=r_single, loss_sets=float(ls[0][0]), loss_single_label=float(l1[0][0])))
            print(f"  step {step + 1:5d}: loss {ls[0][0]:.4f} / {l1[0][0]:.4f}  recall@{args.k}: label sets {r_sets:.4f}, one label per sample {r_single:.4f}")
    excl_pop = []
    for i in range(len(ev["user_id"])):
        seen = set(ev["excl_item_id"][i, :ev["excl_len"][i]].tolist())
        top = [j for j in pop[:args.k + len(seen)] if j not in seen][:args.k]
        pos = ev["pos_item_id"][i, :ev["pos_len"][i]]
        excl_pop.append(np.isin(pos, top).sum() / min(args.k, len(pos)))
    print(f"  popularity: recall@{args.k} {float(np.mean(excl_pop)):.4f}")
    print(f"  host time per step, ids from the host, calls synchronised: label sets {1e3 * t_sets / args.steps:.2f} ms, one label {1e3 * t_single / args.steps:.2f} ms")
    if args.out:
        doc = dict(workload=f"{NU // 2} training users, {len(ev['user_id'])} held-out users, {NI} items, D=64, B={args.batch}, Adam(0.005), dropout 0.5, "
                            f"{args.steps} steps, k={args.k}", start=start, popularity=float(np.mean(excl_pop)), curve=curve,
                   ms_per_step_host_clock=dict(label_sets=1e3 * t_sets / args.steps, one_label=1e3 * t_single / args.steps))
        with open(args.out, "w") as fh:
            json.dump({"multdae_synthetic": doc}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
