#!/usr/bin/env python3
"""The error of `rt.als_half_step` against float64 on every shared case of tests/als_cases.py, as a multiple of the float32
yardstick's error on the same case (tests/test_gpu_als.py asserts ratio <= 4; this script only records).  One record per case
and half: err = max|x - x64| / max|x64|, e32 the same for NumPy's float32 half-step, ratio = err / e32.  Results go to `--out`,
profiles/als_accuracy.json.

    python scripts/als_accuracy.py [--out profiles/als_accuracy.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_accuracy.json"))
    a = ap.parse_args()
    import numpy as np
    import als_cases as ac
    import als_ref as ar
    from openrec_amd import runtime as rt

    def run(name, h):
        F = rt.Table(*h["F"].shape).write(h["F"]); X = rt.Table(*h["X0"].shape).write(h["X0"])
        rt.als_half_step(F, X, rt.ALSCsr(h["ptr"], h["cols"], h["conf"], h["F"].shape[0]), h["a"], h["b"], h["reg"])
        x = X.read()
        err = ar.err_vs(x, h["x64"])
        rec = dict(case=name, err=err, e32=h["e32"], ratio=err / h["e32"], finite=bool(np.isfinite(x).all()))
        print(json.dumps(rec), flush=True)
        return rec

    recs = []
    for k, c in enumerate(ac.ACC_CASES):
        for side, h in ac.accuracy_case(k).items():
            recs.append(run(f"{ac.case_id(c)}-{side}", h))
    recs.append(run("per-entry-conf", ac.conf_case()))
    recs.append(run("long-rows", ac.long_case(rt.als_segment_len())))
    worst = max(recs, key=lambda r: r["ratio"])
    doc = {"als_accuracy": {"bound": ac.FACTOR, "segment_len": rt.als_segment_len(), "largest_ratio": worst["ratio"],
                            "largest_ratio_case": worst["case"], "cases": recs}}
    print("largest ratio %.3g (%s)" % (worst["ratio"], worst["case"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
