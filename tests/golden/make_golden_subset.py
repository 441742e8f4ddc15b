"""Fixtures of train steps over a SUBSET of a model's variables from the reference's own class text:
tests/golden/refstub/{bpr,ucml,wrmf}sub_<roles>_d64_<opt>_s0.npz.

    python tests/golden/make_golden_subset.py [--backend stub] [--reference /root/reference] [--out tests/golden/refstub]

The reference's BPR, UCML and WRMF (recommenders/bpr.py:5-37, ucml.py:7-42, wrmf.py:7-34) are imported from the reference
tree and called, not copied.  The train step is tf2_examples/bpr_citeulike.py:33-39 with one change: `tape.gradient` and
`apply_gradients` get a subset of `model.trainable_variables` -- the variables of the roles in the file name (u = user table,
i = item table, b = item bias).  Keras then updates those variables only; the others, and their optimizer slots, stay as they
were.  Two steps per case, the inputs and the .npz schema of make_golden_tf.run_pair_case; `roles` names the trained roles,
slot_* exist for trained variables only.  Runs only where the reference exists."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_tf import OPT_CLASS, OPTS, SLOTS, load_backend, to_np      # noqa: E402

ROLE_KEY = {"u": "U", "i": "V", "b": "b"}
CASES = [("bpr", "u", "sgd"), ("bpr", "u", "adam"), ("bpr", "ib", "adagrad"),
         ("ucml", "u", "adam"), ("ucml", "ib", "sgd"), ("ucml", "ub", "adagrad"),
         ("wrmf", "u", "sgd"), ("wrmf", "i", "adam")]


def case_name(model_name, roles, optkind, D=64, seed=0):
    return "%ssub_%s_d%d_%s_s%d" % (model_name, roles, D, optkind, seed)


def run_case(tf, rec, model_name, roles, optkind, D=64, seed=0, steps=2):
    from make_golden import make_inputs
    inp = make_inputs(seed, D)
    NU, NI = inp["U"].shape[0], inp["V"].shape[0]
    kw = dict(dim_user_embed=D, dim_item_embed=D, total_users=NU, total_items=NI)
    model = {"bpr": lambda: rec.BPR(**kw), "ucml": lambda: rec.UCML(margin=0.5, **kw), "wrmf": lambda: rec.WRMF(a=2.0, b=0.5, **kw)}[model_name]()
    fdt = np.float64 if "float64" in str(getattr(tf, "float32", "")) else np.float32
    ids = lambda a: tf.constant(a.astype(np.int32), dtype=tf.int32)
    lab = lambda a: tf.constant(a.astype(fdt))
    pointwise = model_name == "wrmf"
    model(*((ids(inp["uid"]), ids(inp["pid"]), lab(inp["label"])) if pointwise else (ids(inp["uid"]), ids(inp["pid"]), ids(inp["nid"]))))
    layers = {"U": model.user_latent_factor, "V": model.item_latent_factor, "b": model.item_bias}
    for k, layer in layers.items():
        layer.set_weights([inp[k].astype(fdt)])
    trained = [ROLE_KEY[r] for r in roles]
    want = {id(layers[k].trainable_variables[0]) for k in trained}
    opt = getattr(tf.keras.optimizers, OPT_CLASS[optkind])(**OPTS[optkind])
    losses = []
    for s in range(steps):       # step s uses the ids rolled as in make_golden_tf.run_pair_case
        u_, p_, n_, l_ = np.roll(inp["uid"], s), np.roll(inp["pid"], 2 * s), np.roll(inp["nid"], 3 * s), np.roll(inp["label"], s)
        args = (ids(u_), ids(p_), lab(l_)) if pointwise else (ids(u_), ids(p_), ids(n_))
        with tf.GradientTape() as tape:
            out = model(*args)
        tv = [v for v in model.trainable_variables if id(v) in want]       # the subset, in the model's order
        assert len(tv) == len(trained)
        opt.apply_gradients(zip(tape.gradient(out, tv), tv))
        losses.append([float(to_np(out[0])), float(to_np(out[1]))])
    res = {("in_" + k): v for k, v in inp.items() if k != "w"}
    for k, layer in layers.items():
        res["out_" + k] = to_np(layer.variables[0]).astype(np.float32)
        if k in trained:
            for slot, short in SLOTS[optkind]:
                res["slot_%s_%s" % (k, short)] = to_np(opt.get_slot(layer.variables[0], slot)).astype(np.float32)
    res["losses"] = np.array(losses, np.float64)
    res["steps"] = np.array(steps)
    res["roles"] = np.array(roles)
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
    for model_name, roles, ok in CASES:
        name = case_name(model_name, roles, ok)
        if args.only and args.only not in name:
            continue
        fn = os.path.join(args.out, name + ".npz")
        np.savez_compressed(fn, **run_case(tf, rec, model_name, roles, ok), **stamp)
        written.append(fn)
        print(fn, os.path.getsize(fn))
    return written


if __name__ == "__main__":
    main()
