#!/usr/bin/env python3
"""examples/seqrec_synthetic.py's data and model, trained on the reference's objective: the softmax of the next item over ALL items
(`VanillaYouTubeRec.train_steps_full`) -- no negatives are drawn, no B x items matrix exists.  Beside it, from the same start and
on the same batches, the sampled-softmax run of that example (`train_steps`, N drawn negatives).  Both are trained on one half
of the users and recommend for the OTHER half from their histories alone; the script prints Recall@K of the held-out users' last
item for both.

    python examples/seqrec_full_softmax.py [--steps 300] [--k 20]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seqrec_synthetic import planted, recall_at                           # noqa: E402
from openrec_amd import runtime as rt                                     # noqa: E402
from openrec_amd.tf2 import data                                          # noqa: E402
from openrec_amd.tf2.recommenders import VanillaYouTubeRec                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--negatives", type=int, default=16)
    ap.add_argument("--seq", type=int, default=5)
    ap.add_argument("--k", type=int, default=20)
    args = ap.parse_args()
    raw, NU, NI = planted()
    train_half = raw["user_id"] % 2 == 0
    train, held = raw[train_half], raw[~train_half]
    ev = next(data.temporal_evaluation(held, NU, args.seq, time_field="ts"))

    def model():
        return VanillaYouTubeRec(dim_item_embed=32, max_seq_len=args.seq, total_items=NI, l2_reg_embed=1e-5, pool="mean")
    full, sampled = model(), model()
    for a, c in zip(full._factors(), sampled._factors()):                 # the same start
        c.table.write(a.table.read())
    opt_full, opt_sampled = rt.Optimizer.adam(0.01), rt.Optimizer.adam(0.01)
    rng = np.random.default_rng(1)
    geo = rt.fullsoftmax_geometry(args.batch, NI, 32)
    print(f"{train.size} training records of {NU // 2} users, {len(ev['label'])} held-out users, {NI} items, histories of up to {args.seq}, "
          f"D = 32, B = {args.batch}, Adam(0.01)")
    print(f"  full softmax: {geo['item_chunks']} item chunks, {geo['sample_chunks']} sample chunks, {geo['scratch_bytes'] / 2 ** 20:.1f} MiB of "
          f"scratch (a B x items logit matrix and its gradient: {2 * args.batch * NI * 4 / 2 ** 20:.1f} MiB)")
    print(f"  start     : recall@{args.k} for the held-out users {recall_at(full, ev, args.k):.4f}")
    batches = data.temporal_batches(train, NU, args.batch, args.seq, seed=2, time_field="ts")
    for step in range(args.steps):
        bt = next(batches)
        nid = rng.integers(0, NI, (args.batch, args.negatives)).astype(np.int32)
        want = (step + 1) % 100 == 0
        lf = full.train_steps_full(opt_full, bt["seq_item_id"], bt["seq_len"], bt["label"], want_loss=want)
        ls = sampled.train_steps(opt_sampled, bt["seq_item_id"], bt["seq_len"], bt["label"], nid, loss="softmax", want_loss=want)
        if want or step + 1 == args.steps:
            tail = f"loss {lf[0][0]:.4f} / {ls[0][0]:.4f}  " if lf is not None else ""
            print(f"  step {step + 1:5d}: {tail}recall@{args.k} for the held-out users: full softmax {recall_at(full, ev, args.k):.4f}, "
                  f"sampled softmax (N = {args.negatives}) {recall_at(sampled, ev, args.k):.4f}")


if __name__ == "__main__":
    main()
