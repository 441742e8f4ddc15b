#!/usr/bin/env python3
"""The error of the CG half-step (`rt.als_half_step(..., solver="cg")`) against the float64 recurrence on every shared case of
tests/als_cg_cases.py at 1, 2 and 3 steps, as a multiple of the float32 yardstick's error on the same case and step count
(tests/test_gpu_als_cg.py asserts ratio <= FACTOR_CG; this script only records).  One record per case, half and step count:
err = max|x - cg64| / max|cg64|, e32cg the same for the float32 recurrence, ratio = err / e32cg.  A largest ratio above 4 says that
more of the recurrence belongs in fp64.  Results go to `--out`, profiles/als_cg_accuracy.json.

    python scripts/als_cg_accuracy.py [--out profiles/als_cg_accuracy.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_cg_accuracy.json"))
    a = ap.parse_args()
    import numpy as np
    import als_cg_cases as cc
    import als_ref as ar
    from openrec_amd import runtime as rt

    def run(name, h):
        F = rt.Table(*h["F"].shape).write(h["F"]); X = rt.Table(*h["X0"].shape).write(h["X0"])
        rt.als_half_step(F, X, rt.ALSCsr(h["ptr"], h["cols"], h["conf"], h["F"].shape[0]), h["a"], h["b"], h["reg"],
                         solver="cg", cg_steps=h["steps"])
        x = X.read()
        err = ar.err_vs(x, h["x64"])
        rec = dict(case=name, steps=h["steps"], err=err, e32cg=h["e32cg"], ratio=err / h["e32cg"], finite=bool(np.isfinite(x).all()))
        print(json.dumps(rec), flush=True)
        return rec

    recs = [run(cc.half_id(w), cc.solved(w, s)) for w in cc.HALVES for s in cc.CG_STEPS]
    breaks, L = rt.als_cg_row_breaks(64), rt.als_segment_len()
    recs.append(run("long-rows-and-breaks", cc.breaks_case(tuple(breaks), L)))
    worst = max(recs, key=lambda r: r["ratio"])
    doc = {"als_cg_accuracy": {"bound": cc.FACTOR_CG, "row_breaks_D64": breaks, "largest_ratio": worst["ratio"],
                               "largest_ratio_case": "%s, %d steps" % (worst["case"], worst["steps"]), "cases": recs}}
    print("largest ratio %.3g (%s, %d steps)" % (worst["ratio"], worst["case"], worst["steps"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
