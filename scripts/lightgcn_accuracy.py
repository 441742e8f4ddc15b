#!/usr/bin/env python3
"""How close the device's graph propagation is to float64, next to a float32 NumPy evaluation of the same cases
(tests/lightgcn_cases.py GEN_CASES: 300 x 200, Zipf items, D in {16, 64}, L in {1, 3}).  The tests hold the device to the
worst-case bound L (n_max + 8) u P(|U|, |V|), which a float32 evaluation uses a few thousandths of; this script records the
figure the bound cannot see: max|got - ref64| / max|ref64| of the device and of NumPy float32 adding a row's terms in CSR order
and in the reverse order.  No threshold.  Results go to `--out`, profiles/lightgcn_accuracy.json.

    python scripts/lightgcn_accuracy.py [--out profiles/lightgcn_accuracy.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lightgcn_accuracy.json"))
    args = ap.parse_args()
    import lightgcn_cases as lc
    import lightgcn_ref as lr
    from openrec_amd import runtime as rt

    def rel(got, ref):
        return float(max(np.abs(g.astype(np.float64) - r).max() for g, r in zip(got, ref)) / max(np.abs(r).max() for r in ref))

    cases = []
    for D, L in lc.GEN_CASES:
        h = lc.general_case(D, L)
        graph = rt.InteractionGraph(lr.records_of(*h["by_user"]), lc.GEN_NU, lc.GEN_NI)
        U = rt.Table(*h["U"].shape).write(h["U"]); V = rt.Table(*h["V"].shape).write(h["V"])
        Uf, Vf = rt.LightGCN(U, V, graph, layers=L).propagate()
        ref = (h["fu"], h["fv"])
        f32 = [lr.propagate(h["U"], h["V"], h["by_user"], h["by_item"], h["su"], h["sv"], h["al"], np.float32, reverse=rev) for rev in (False, True)]
        dev = (Uf.read(), Vf.read())
        used = max(float((np.abs(g.astype(np.float64) - r)[b > 0] / b[b > 0]).max()) for g, r, b in zip(dev, ref, (h["bu"], h["bv"])))
        cases.append(dict(D=D, L=L, n_max=h["n_max"], device=rel(dev, ref), numpy_f32=rel(f32[0], ref), numpy_f32_reversed=rel(f32[1], ref),
                          device_share_of_bound=used))
        print(cases[-1])
    worst = max(c["device"] / max(c["numpy_f32"], c["numpy_f32_reversed"]) for c in cases)
    res = dict(cases=cases, device_over_numpy_f32_worst=worst)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("device / float32 NumPy, worst case:", round(worst, 3))


if __name__ == "__main__":
    main()
