#!/usr/bin/env python3
"""YouTubeRec (user-feature embeddings and a hidden layer in front of the softmax over all items) against the depth-0
VanillaYouTubeRec on a synthetic set that the depth-0 model cannot fit: items come in G groups; a history holds items of two
groups (a, c); the next item lies in group (a * c + 3 * gender) mod G -- a product of the history's groups, shifted by a user
feature the depth-0 model never sees -- and `geo` picks which part of that group.  Both models train on the softmax over all
items (`train_steps_full`) from the same batches and recommend for held-out histories; the script prints Recall@K for both.

    python examples/youtube_rec_synthetic.py [--steps 400] [--k 20]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openrec_amd import runtime as rt                                     # noqa: E402
from openrec_amd.tf2.recommenders import VanillaYouTubeRec, YouTubeRec    # noqa: E402

G, PER, GEO = 16, 40, 4                       # groups, items per group, values of `geo`


def draw(rng, n, L):
    """-> seq [n, L], seq_len [n], gender [n], geo [n], label [n]"""
    a, c = rng.integers(1, G, n), rng.integers(1, G, n)
    gender, geo = rng.integers(0, 2, n), rng.integers(0, GEO, n)
    lens = rng.integers(2, L + 1, n)
    pick = rng.integers(0, 2, (n, L))                                     # each position from group a or group c, both present
    pick[:, 0], pick[:, 1] = 0, 1
    seq = (np.where(pick == 0, a[:, None], c[:, None]) * PER + rng.integers(0, PER, (n, L))).astype(np.int32)
    target = (a * c + 3 * gender) % G
    part = PER // GEO
    label = (target * PER + geo * part + rng.integers(0, part, n)).astype(np.int32)
    return seq, lens.astype(np.int32), gender.astype(np.int32), geo.astype(np.int32), label


def recall_at(model, held, k, feats):
    seq, lens, gender, geo, label = held
    ids, _ = model.recommend(seq, lens, k, **(dict(gender=gender, geo=geo) if feats else {}))
    return float((np.asarray(ids) == label[:, None]).any(1).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--seq", type=int, default=6)
    ap.add_argument("--k", type=int, default=20)
    args = ap.parse_args()
    NI = G * PER
    rng = np.random.default_rng(0)
    held = draw(rng, 4096, args.seq)
    deep = YouTubeRec(user_dict={"gender": 2, "geo": GEO}, item_dict={"id": NI}, dim_user_embed={"gender": 4, "geo": 4, "total": 8},
                      dim_item_embed={"id": 32, "total": 32}, max_seq_len=args.seq, hidden=[128, 32], pool="mean")
    flat = VanillaYouTubeRec(dim_item_embed=32, max_seq_len=args.seq, total_items=NI, use_item_bias=False, pool="mean")
    od, of = rt.Optimizer.adam(0.01), rt.Optimizer.adam(0.01)
    print(f"{NI} items in {G} groups, histories of up to {args.seq}, B = {args.batch}, Adam(0.01); tower {deep._net.widths}, "
          f"{rt.tower_geometry(args.batch, deep._net.widths)['scratch_bytes'] / 2 ** 20:.1f} MiB of tower scratch")
    print(f"  start     : recall@{args.k} tower {recall_at(deep, held, args.k, True):.4f}, depth 0 {recall_at(flat, held, args.k, False):.4f}")
    for step in range(args.steps):
        seq, lens, gender, geo, label = draw(rng, args.batch, args.seq)
        want = (step + 1) % 100 == 0 or step + 1 == args.steps
        ld = deep.train_steps_full(od, seq, lens, label, want_loss=want, gender=gender, geo=geo)
        lf = flat.train_steps_full(of, seq, lens, label, want_loss=want)
        if want:
            print(f"  step {step + 1:5d}: loss {ld[0][0]:.4f} / {lf[0][0]:.4f}  recall@{args.k} tower {recall_at(deep, held, args.k, True):.4f}, "
                  f"depth 0 {recall_at(flat, held, args.k, False):.4f}")


if __name__ == "__main__":
    main()
