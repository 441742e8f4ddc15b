#!/usr/bin/env python3
"""The time of the N-negative step (`rt.multineg_step`) at 1M x 1M x 64, B = 65 536, K = 20 per call, SGD with the item bias, ids
resident in HBM, no loss read-back: both losses at N in {4, 16}, and -- for context only -- N plain `rt.pairwise_step` calls over
the same positives, which is a DIFFERENT objective (N optimizer steps, no normalisation across the negatives) and therefore a
yardstick, not a bar.  One process, the forms interleaved call by call on tables of their own, a host clock around synchronised
calls; per form the median time per step over the timed calls and their spread (max - min).  The measuring process runs as a
child under a time limit of its own; a failure ends the script.  Results go to `--out`, profiles/multineg_bench.json.

    python scripts/multineg_bench.py [--calls 7] [--warmup 3] [--out profiles/multineg_bench.json]
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
D, B, K = 64, 65536, 20
GS = (D + 1 + 3) // 4 * 4                     # floats per gradient row (the bias gradient in column D)


def algorithmic_bytes(N, softmax):
    """per sample, from the shapes: what the gradient launch and the two applies must move at the least (the sort of the id lists
    and the second read of the negative rows by the softmax, which L2 serves, are listed apart)"""
    rows = 2 + N
    grads = dict(ids=4 * rows, rows_read=4 * D * rows, biases_read=4 * (1 + N), gradient_rows_written=4 * GS * rows, item_list_written=4 * (1 + N))
    apply = dict(gradient_rows_read=4 * GS * rows, ids_read=4 * rows, rows_read_modify_write=2 * 4 * D * rows, biases_read_modify_write=2 * 4 * (1 + N))
    out = dict(gradient_launch=sum(grads.values()), applies=sum(apply.values()))
    out["total"] = out["gradient_launch"] + out["applies"]
    out["second_read_of_negative_rows_from_L2"] = 4 * D * N if softmax else 0
    return out


def measure(calls, warmup):
    import torch
    from openrec_amd import runtime as rt
    torch.manual_seed(0)
    ctx = rt.default_context()
    forms = []
    for N in (4, 16):
        for kind in ("softmax", "logsig", "pairwise_x_N"):
            tU = rt.Table(NU, D).init_uniform(seed=1); tV = rt.Table(NI, D).init_uniform(seed=2); tb = rt.Table(NI, 1).init_uniform(seed=3)
            forms.append(dict(name=f"{kind}_N{N}", kind=kind, N=N, tables=(tU, tV, tb), o=rt.Optimizer.sgd(0.05), us=[]))

    def call(f):
        N = f["N"]
        uid = torch.randint(0, NU, (K, B), dtype=torch.int32, device="cuda")
        pid = torch.randint(0, NI, (K, B), dtype=torch.int32, device="cuda")
        nid = torch.randint(0, NI, (K, B, N), dtype=torch.int32, device="cuda")
        cols = [nid[:, :, j].contiguous() for j in range(N)] if f["kind"] == "pairwise_x_N" else None
        torch.cuda.synchronize(); ctx.synchronize()
        t0 = time.perf_counter()
        if cols is None:
            rt.multineg_step(f["kind"], f["o"], *f["tables"], uid, pid, nid, K=K, B=B, want_loss=False)
        else:
            for c in cols:
                rt.pairwise_step("bpr", f["o"], *f["tables"], uid, pid, c, K=K, B=B, want_loss=False)
        ctx.synchronize()
        return (time.perf_counter() - t0) / K * 1e6

    for it in range(warmup + calls):            # interleaved: every form sees the same box at the same time
        for f in forms:
            dt = call(f)
            if it >= warmup:
                f["us"].append(dt)
    out = {"workload": "D=%d %dx%d B=%d K=%d SGD with the item bias, ids on the device, no read-back" % (D, NU, NI, B, K),
           "calls": calls, "warmup": warmup,
           "note": "pairwise_x_N: N plain pairwise_step calls of K steps over the same positives -- a different objective, quoted as a yardstick only; its time is per K-step group of N calls divided by K"}
    for f in forms:
        out[f["name"]] = {"us_per_step_median": statistics.median(f["us"]), "us_per_step_spread": max(f["us"]) - min(f["us"]),
                          "us_per_step": [round(t, 2) for t in f["us"]]}
        if f["kind"] != "pairwise_x_N":
            out[f["name"]]["algorithmic_bytes_per_sample"] = algorithmic_bytes(f["N"], f["kind"] == "softmax")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multineg_bench.json"))
    ap.add_argument("--limit", type=int, default=300, help="seconds the measuring process may take")
    ap.add_argument("--measure", action="store_true", help="(the child) measure in this process and print one JSON line")
    a = ap.parse_args()
    if a.measure:
        print(json.dumps(measure(a.calls, a.warmup)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--measure", "--calls", str(a.calls), "--warmup", str(a.warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    sys.stderr.write(r.stderr[-2000:])
    if r.returncode != 0:
        print("the measuring process failed with status %d" % r.returncode)
        return r.returncode
    doc = {"multineg_step": json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])}
    print(json.dumps(doc["multineg_step"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
