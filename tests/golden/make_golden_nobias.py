"""Fixtures of BPR WITHOUT item biases from the reference's own module text: tests/golden/refstub/bprnb_*.npz.

    python tests/golden/make_golden_nobias.py [--backend stub] [--reference /root/reference] [--out tests/golden/refstub]

The reference has no bias-free recommender, but its PairwiseLogLoss takes the two item biases as optional arguments
(openrec/tf2/modules/pairwise_log_loss.py:6, :26-30).  The model below is the reference's BPR (recommenders/bpr.py:22-37) written
out by hand without the item_bias factor: three lookups of the reference's LatentFactor, PairwiseLogLoss with no biases, and
tf.nn.l2_loss of the three lookups.  LatentFactor and PairwiseLogLoss are imported from the reference tree and called, not
copied; the backend and the train step come from make_golden_tf.py.  Cases: SGD, Adagrad and Adam at D in {50, 64}, two steps,
the inputs and the .npz schema of make_golden_tf.run_pair_case without its bias entries.  Runs only where the reference exists."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_tf import OPT_CLASS, OPTS, SLOTS, load_backend, to_np, train_step      # noqa: E402

CASES = [(D, ok) for D in (50, 64) for ok in ("sgd", "adagrad", "adam")]


def bias_free_bpr(tf, modules, D, NU, NI):
    """recommenders/bpr.py:5-37 without item_bias"""
    class BiasFreeBPR(tf.keras.Model):
        def __init__(self):
            super().__init__()
            self.user_latent_factor = modules.LatentFactor(num_instances=NU, dim=D, name='user_latent_factor')
            self.item_latent_factor = modules.LatentFactor(num_instances=NI, dim=D, name='item_latent_factor')
            self.pairwise_log_loss = modules.PairwiseLogLoss()

        def call(self, user_id, p_item_id, n_item_id):
            user_vec = self.user_latent_factor(user_id)
            p_item_vec = self.item_latent_factor(p_item_id)
            n_item_vec = self.item_latent_factor(n_item_id)
            loss = self.pairwise_log_loss(user_vec=user_vec, p_item_vec=p_item_vec, n_item_vec=n_item_vec)
            l2_loss = tf.nn.l2_loss(user_vec) + tf.nn.l2_loss(p_item_vec) + tf.nn.l2_loss(n_item_vec)
            return loss, l2_loss
    return BiasFreeBPR()


def run_case(tf, modules, D, optkind, seed=0, steps=2):
    from make_golden import make_inputs
    inp = make_inputs(seed, D)
    NU, NI = inp["U"].shape[0], inp["V"].shape[0]
    model = bias_free_bpr(tf, modules, D, NU, NI)
    fdt = np.float64 if "float64" in str(getattr(tf, "float32", "")) else np.float32
    ids = lambda a: tf.constant(a.astype(np.int32), dtype=tf.int32)
    model(ids(inp["uid"]), ids(inp["pid"]), ids(inp["nid"]))          # builds the layers
    model.user_latent_factor.set_weights([inp["U"].astype(fdt)])
    model.item_latent_factor.set_weights([inp["V"].astype(fdt)])
    opt = getattr(tf.keras.optimizers, OPT_CLASS[optkind])(**OPTS[optkind])
    losses = []
    for s in range(steps):       # step s uses the ids rolled as in make_golden_tf.run_pair_case
        u_, p_, n_ = np.roll(inp["uid"], s), np.roll(inp["pid"], 2 * s), np.roll(inp["nid"], 3 * s)
        out, _ = train_step(tf, model, opt, ids(u_), ids(p_), ids(n_))
        losses.append([float(to_np(out[0])), float(to_np(out[1]))])
    res = {("in_" + k): inp[k] for k in ("U", "V", "uid", "pid", "nid")}
    for k, layer in (("U", model.user_latent_factor), ("V", model.item_latent_factor)):
        res["out_" + k] = to_np(layer.variables[0]).astype(np.float32)
        for slot, short in SLOTS[optkind]:
            res["slot_%s_%s" % (k, short)] = to_np(opt.get_slot(layer.variables[0], slot)).astype(np.float32)
    res["losses"] = np.array(losses, np.float64)
    res["steps"] = np.array(steps)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--backend", choices=("tf", "stub"), default="stub")
    ap.add_argument("--dtype", choices=("float32", "float64"), default="float64", help="stub only (TensorFlow runs float32)")
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "refstub"))
    ap.add_argument("--only", default=None, help="substring filter on case names")
    args = ap.parse_args(argv)
    os.makedirs(args.out, exist_ok=True)
    tf, _ = load_backend(args.backend, args.dtype, args.reference)
    from openrec.tf2 import modules
    stamp = dict(dtype=np.array("float32" if args.backend == "tf" else args.dtype), backend=np.array("%s %s" % (args.backend, tf.__version__)))
    written = []
    for D, ok in CASES:
        name = "bprnb_d%d_%s_s0" % (D, ok)
        if args.only and args.only not in name:
            continue
        fn = os.path.join(args.out, name + ".npz")
        np.savez_compressed(fn, **run_case(tf, modules, D, ok), **stamp)
        written.append(fn)
        print(fn, os.path.getsize(fn))
    return written


if __name__ == "__main__":
    main()
