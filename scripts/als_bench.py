#!/usr/bin/env python3
"""The time of an ALS sweep of WRMF (`rt.als_half_step`) at 1M users x 1M items, about 20M observations, items ~ Zipf(1.05) and
users uniform, the CSRs resident in HBM: per user half-step, per item half-step and per sweep at D = 64 and D = 128, and the
same at D = 64 with the items uniform (what the skew and the segment path cost).  One process; per figure the median of `--calls`
synchronised calls after `--warmup`, a host clock around them, with the spread (max - min).  Next to the times:

  gram        the item half-step over ONE row (the shortest; empty under the Zipf draw) is the gram kernel over the user table, its
              reduction and a one-workgroup solver launch: its time against the bytes of the fixed table, which the gram reads once,
              next to the float4-copy rate `ctx.copy_bandwidth` measures in the same process (reads + writes: a pure read stream
              at that rate moves half of it)
  rank rate   2 nnz D^2 FLOP per half-step (the full squares; the kernels form the lower triangles only) over the half-step's
              time, against the 157 TF fp32 matrix peak
  split       a row's cost modelled as t0 + chunks x tc and fitted on synthetic CSRs of 262144 rows with exactly 32 / 64 / 128
              observations per row (1 / 2 / 4 chunks of 32 gathered rows): t0 is the factorisation, the substitutions and the
              fixed parts, tc the accumulation of one chunk; the share of accumulation in a real half-step is
              (its chunks x tc) / its time

The measuring process runs as a child under a time limit of its own; a failure ends the script.  Results go to `--out`,
profiles/als_bench.json.

    python scripts/als_bench.py [--calls 5] [--warmup 2] [--out profiles/als_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NU = NI = 1_000_000
NNZ = 20_000_000
PEAK_TF = 157.3
CH = 32                     # gathered rows per chunk (kernels_als.hip ALS_CH)


def records(zipf, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    users = rng.integers(0, NU, NNZ, dtype=np.int64)
    if zipf:
        cdf = np.cumsum(np.arange(1, NI + 1, dtype=np.float64) ** -1.05)
        cdf /= cdf[-1]
        items = rng.permutation(NI)[np.searchsorted(cdf, rng.random(NNZ))]
    else:
        items = rng.integers(0, NI, NNZ, dtype=np.int64)
    rec = np.zeros(NNZ, dtype=[("user_id", np.int32), ("item_id", np.int32)])
    rec["user_id"], rec["item_id"] = users, items
    return rec


def measure(calls, warmup):
    import numpy as np
    import torch
    from openrec_amd import runtime as rt
    ctx = rt.default_context()
    L = rt.als_segment_len()

    def timed(fn):
        ts = []
        for it in range(warmup + calls):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            if it >= warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        return dict(ms_median=statistics.median(ts), ms_spread=max(ts) - min(ts), ms=[round(t, 3) for t in ts])

    def chunks(csr):
        n = np.diff(csr.ptr)
        return int(((n + CH - 1) // CH).sum())

    def fit_split(D):
        """t0 and tc per row (ns) from synthetic CSRs with exactly c observations per row"""
        R, M = 262144, 262144
        F = rt.Table(M, D).init_uniform(seed=5); X = rt.Table(R, D).init_uniform(seed=6)
        pts = []
        for c in (32, 64, 128):
            stride = M // c
            start = np.random.default_rng(c).integers(0, stride, R)
            cols = (start[:, None] + np.arange(c)[None, :] * stride).astype(np.int32).reshape(-1)      # ascending, distinct
            csr = rt.ALSCsr(np.arange(R + 1, dtype=np.int64) * c, cols, None, M).to_device(ctx)
            t = timed(lambda: rt.als_half_step(F, X, csr, 5.0, 1.0, 0.1))
            pts.append((c // CH, t["ms_median"] * 1e6 / R))
        k = np.array([p[0] for p in pts], np.float64); y = np.array([p[1] for p in pts], np.float64)
        tc, t0 = np.polyfit(k, y, 1)
        return dict(rows=R, ns_per_row_at_chunks={str(int(a)): round(b, 1) for a, b in pts}, t0_ns_per_row=float(t0), tc_ns_per_chunk=float(tc))

    out = {"workload": "%d x %d, %d records before duplicates merge, confidences a = 5, b = 1, reg = 0.1, CSRs on the device" % (NU, NI, NNZ),
           "calls": calls, "warmup": warmup, "segment_len": L}
    out["copy_GBps_read_plus_write"] = ctx.copy_bandwidth()
    splits = {D: fit_split(D) for D in (64, 128)}
    out["split_fit"] = {str(D): s for D, s in splits.items()}
    for name, zipf, dims in (("zipf_1.05", True, (64, 128)), ("uniform", False, (64,))):
        data = rt.ALSData(records(zipf), NU, NI, ctx=ctx)
        lens = np.diff(data.by_item.ptr)
        res = {"nnz": data.nnz, "longest_item_row": int(lens.max()), "item_rows_over_segment_len": int((lens > L).sum()),
               "item_segments": int(((lens[lens > L] + L - 1) // L).sum())}
        for D in dims:
            U = rt.Table(NU, D).init_uniform(seed=1); V = rt.Table(NI, D).init_uniform(seed=2)
            r = {}
            r["user_half"] = timed(lambda: rt.als_half_step(V, U, data.by_user, 5.0, 1.0, 0.1))
            r["item_half"] = timed(lambda: rt.als_half_step(U, V, data.by_item, 5.0, 1.0, 0.1))
            r["sweep"] = timed(lambda: rt.als_sweep(U, V, data, 5.0, 1.0, 0.1))
            short = int(np.argmin(lens))                    # the item half-step over this one row: the gram of U and next to nothing else
            g = timed(lambda: rt.als_half_step(U, V, data.by_item, 5.0, 1.0, 0.1, rows=(short, 1)))
            gb = NU * D * 4 / 1e9                           # the fixed table, read once
            r["gram_plus_one_row"] = dict(g, row_len=int(lens[short]), fixed_table_GB=gb, GBps_read=gb / (g["ms_median"] * 1e-3),
                                          copy_GBps_read_plus_write=out["copy_GBps_read_plus_write"],
                                          ms_reading_at_half_the_copy_rate=gb / (out["copy_GBps_read_plus_write"] / 2) * 1e3)
            s = splits[D]
            for half, csr in (("user_half", data.by_user), ("item_half", data.by_item)):
                t = r[half]["ms_median"] * 1e-3
                r[half]["rank_update_TF"] = 2.0 * data.nnz * D * D / t / 1e12
                r[half]["rank_update_share_of_peak"] = r[half]["rank_update_TF"] / PEAK_TF
                r[half]["chunks"] = chunks(csr)
                r[half]["accumulation_share_by_fit"] = r[half]["chunks"] * s["tc_ns_per_chunk"] * 1e-9 / t
            res["D%d" % D] = r
            print(name, D, json.dumps({k: v.get("ms_median") for k, v in r.items()}), file=sys.stderr, flush=True)
            del U, V
        out[name] = res
        del data
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_bench.json"))
    ap.add_argument("--limit", type=int, default=540, help="seconds the measuring process may take")
    ap.add_argument("--measure", action="store_true", help="(the child) measure in this process and print one JSON line")
    a = ap.parse_args()
    if a.measure:
        print(json.dumps(measure(a.calls, a.warmup)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--measure", "--calls", str(a.calls), "--warmup", str(a.warmup)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        print("the measuring process failed with status %d" % r.returncode)
        return r.returncode
    doc = {"als_bench": json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])}
    print(json.dumps(doc["als_bench"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
