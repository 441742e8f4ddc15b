"""Fixtures of train steps with an L2 COEFFICIENT from the reference's own class text:
tests/golden/refstub/{bpr,ucml,wrmf,gmf}reg_d64_<opt>_s0.npz.

    python tests/golden/make_golden_l2reg.py [--backend stub] [--reference /root/reference] [--out tests/golden/refstub]

The reference's BPR, UCML, WRMF and GMF (recommenders/bpr.py, ucml.py, wrmf.py, gmf.py) are imported from the reference tree and
called, not copied.  The train step is tf2_examples/bpr_citeulike.py:33-39 with one change, the one everybody makes: the target
of `tape.gradient` is `loss + L2_REG * l2_loss` instead of the tuple `(loss, l2_loss)`.  Two steps per case, the inputs and the
.npz schema of make_golden_tf.run_pair_case; `losses` holds (loss, l2_loss) -- l2_loss unscaled --, `l2_reg` the coefficient.
Runs only where the reference exists."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_tf import OPT_CLASS, OPTS, SLOTS, load_backend, to_np      # noqa: E402

L2_REG = 0.01
CASES = [("bpr", "sgd"), ("bpr", "adagrad"), ("bpr", "adam"), ("ucml", "sgd"), ("ucml", "adam"),
         ("wrmf", "sgd"), ("wrmf", "adam"), ("gmf", "sgd"), ("gmf", "adagrad")]


def case_name(model_name, optkind, D=64, seed=0):
    return "%sreg_d%d_%s_s%d" % (model_name, D, optkind, seed)


def run_case(tf, rec, model_name, optkind, D=64, seed=0, steps=2):
    from make_golden import make_inputs
    inp = make_inputs(seed, D)
    NU, NI = inp["U"].shape[0], inp["V"].shape[0]
    kw = dict(dim_user_embed=D, dim_item_embed=D, total_users=NU, total_items=NI)
    model = {"bpr": lambda: rec.BPR(**kw), "ucml": lambda: rec.UCML(margin=0.5, **kw), "wrmf": lambda: rec.WRMF(a=2.0, b=0.5, **kw),
             "gmf": lambda: rec.GMF(**kw)}[model_name]()
    fdt = np.float64 if "float64" in str(getattr(tf, "float32", "")) else np.float32
    ids = lambda a: tf.constant(a.astype(np.int32), dtype=tf.int32)
    lab = lambda a: tf.constant(a.astype(fdt))
    pointwise = model_name in ("wrmf", "gmf")
    model(*((ids(inp["uid"]), ids(inp["pid"]), lab(inp["label"])) if pointwise else (ids(inp["uid"]), ids(inp["pid"]), ids(inp["nid"]))))
    layers = {"U": model.user_latent_factor, "V": model.item_latent_factor, "b": model.item_bias}
    for k, layer in layers.items():
        layer.set_weights([inp[k].astype(fdt)])
    if model_name == "gmf":
        model.mlp.set_weights([inp["w"].astype(fdt)])
    opt = getattr(tf.keras.optimizers, OPT_CLASS[optkind])(**OPTS[optkind])
    losses = []
    for s in range(steps):       # step s uses the ids rolled as in make_golden_tf.run_pair_case
        u_, p_, n_, l_ = np.roll(inp["uid"], s), np.roll(inp["pid"], 2 * s), np.roll(inp["nid"], 3 * s), np.roll(inp["label"], s)
        args = (ids(u_), ids(p_), lab(l_)) if pointwise else (ids(u_), ids(p_), ids(n_))
        with tf.GradientTape() as tape:
            loss, l2 = model(*args)
            target = loss + L2_REG * l2
        tv = model.trainable_variables
        opt.apply_gradients(zip(tape.gradient(target, tv), tv))
        losses.append([float(to_np(loss)), float(to_np(l2))])
    res = {("in_" + k): v for k, v in inp.items() if k != "w" or model_name == "gmf"}
    outs = dict(layers)
    if model_name == "gmf":
        outs["w"] = model.mlp
    for k, layer in outs.items():
        var = layer.trainable_variables[0]
        res["out_" + k] = to_np(var).astype(np.float32)
        for slot, short in SLOTS[optkind]:
            res["slot_%s_%s" % (k, short)] = to_np(opt.get_slot(var, slot)).astype(np.float32)
    res["losses"] = np.array(losses, np.float64)
    res["steps"] = np.array(steps)
    res["l2_reg"] = np.array(L2_REG)
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
    tf, rec = load_backend(args.backend, args.dtype, args.reference)
    stamp = dict(dtype=np.array("float32" if args.backend == "tf" else args.dtype), backend=np.array("%s %s" % (args.backend, tf.__version__)))
    written = []
    for model_name, ok in CASES:
        name = case_name(model_name, ok)
        if args.only and args.only not in name:
            continue
        fn = os.path.join(args.out, name + ".npz")
        np.savez_compressed(fn, **run_case(tf, rec, model_name, ok), **stamp)
        written.append(fn)
        print(fn, os.path.getsize(fn))
    return written


if __name__ == "__main__":
    main()
