"""Child process of tests/test_gpu_plan.py: runs one SET of duplicate-plan cases through orx_plan_dump and tests/plan_ref.check_plan and
writes {case id: "ok" | message} as JSON.  One process per setting that the library reads once (ORX_PLAN_V1).

    python tests/plan_worker.py <set: v2 | v1 | seq> <result.json>
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import plan_ref as R  # noqa: E402

# what a case may end with and still leave the child healthy: a violated rule, or an argument / memory error RETURNED by the library --
# recorded under the case.  A HIP error (the device may have faulted) and anything else end the child: nothing more runs on the card.
CASE_ERRORS = (R.PlanError, AssertionError, ValueError, MemoryError, IndexError)
TPW = {16: 16, 32: 8, 64: 4, 128: 2, 256: 1}          # orx_fused_tpw of the float4 dims (kernels_pairwise.hip lpr_for_dim); 1: no pairing


def geometry(NU, NI, B, pairwise=True):
    from openrec_amd import _ffi
    out = (ctypes.c_int32 * 16)()
    _ffi.check(_ffi.load().orx_plan_geometry(NU, NI, B, B, B if pairwise else 0, out))
    return R.geometry_dict(list(out))


# ---------------------------------------------------------------------------------------------- id structures
def make_ids(case):
    """(uid, pid, nid | None, labels | None) [K][B] of a case, seeded by its id."""
    rng = np.random.default_rng(abs(hash_id(case["id"])))
    K, B, NU, NI, gen = case["K"], case["B"], case["NU"], case["NI"], case["gen"]
    geo = geometry(NU, NI, B, not case.get("pointwise"))

    def zipf(a, rows, size):
        return ((rng.zipf(a, size) - 1) % rows).astype(np.int32)

    def draw(rows, size, nb):
        if gen == "uniform":
            return rng.integers(0, rows, size).astype(np.int32)
        if gen.startswith("zipf"):
            return zipf(float(gen[4:]), rows, size)
        if gen == "hot":
            return np.zeros(size, np.int32)
        if gen == "five":
            return rng.integers(0, min(5, rows), size).astype(np.int32)
        if gen == "runs64":                      # runs of one row that start and end on 64 boundaries
            x = np.repeat(rng.integers(0, rows, (size[0], (size[1] + 63) // 64)), 64, axis=1)[:, :size[1]]
            return x.astype(np.int32)
        if gen == "twice":                       # every referenced row exactly twice
            h = (size[1] + 1) // 2
            x = np.stack([rng.permutation(np.concatenate([np.arange(h), np.arange(h)])[:size[1]] % rows) for _ in range(size[0])])
            return x.astype(np.int32)
        if gen == "onebucket":                   # ids with the same low bits: one range gets every reference
            per = max(1, rows // nb)
            want = case.get("rows_in_bucket", 2000)
            return (rng.integers(0, min(per, want), size) * nb).astype(np.int32)
        if gen == "manytri":                     # more than 65 535 rows of one range referenced three times
            per = rows // nb
            k = np.arange(size[1]) // 3 % per
            return np.stack([rng.permutation(k) * nb for _ in range(size[0])]).astype(np.int32)
        raise ValueError(gen)

    u = draw(NU, (K, B), geo["nru"])
    if gen == "manytri":
        both = draw(NI, (K, 2 * B), geo["nri"])
        p, n = np.ascontiguousarray(both[:, :B]), np.ascontiguousarray(both[:, B:])
    else:
        p, n = draw(NI, (K, B), geo["nri"]), draw(NI, (K, B), geo["nri"])
    if gen == "twice":
        n = (n.astype(np.int64) + (B + 1) // 2).astype(np.int32) % NI if NI > B else n
    if case.get("posneg"):
        n[:, ::3] = p[:, ::3]
    for where in case.get("invalid", ()):
        j = {"first": 0, "last": B - 1, "pair": 5}.get(where, where)
        u[0, j] = -1
        n[K - 1, j] = NI
        if where == "pair" and B >= 8:           # an invalid id next to a row referenced exactly twice
            p[0, 2] = p[0, B - 3] = NI - 1
            p[0, 3] = -5
    lab = None
    if case.get("pointwise"):
        n = None
        lab = rng.random((K, B)).astype(np.float32)
    return u, p, n, lab


def hash_id(s):
    h = 0
    for ch in s:
        h = (h * 131 + ord(ch)) % (1 << 31)
    return h


# ---------------------------------------------------------------------------------------------- the entry point
def plan_dump(ctx, ids, labels, NU, NI, D, opt):
    from openrec_amd import _ffi
    lib = _ffi.load()
    u, p, n = ids
    K, B = u.shape
    o = (ctypes.c_int32 * 8)(opt["version"], int(opt["staging"]), int(opt["urgent"]), opt.get("tpw", 0), opt.get("min_late", -1),
                             int(opt.get("big", 0)), opt.get("step0", 0), 0)
    info = (ctypes.c_int64 * 8)()
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    _ffi.check(lib.orx_plan_dump(ctx, ptr(u), ptr(p), ptr(n), ptr(labels), K, B, NU, NI, D, o, None, info))
    S = int(info[0])
    d = dict(ids=np.zeros((K, 3, B), np.uint32), pword=np.zeros((K, B), np.uint32), dlist=np.zeros((K, 2 * B), np.uint32),
             dcount=np.zeros(K, np.int32), alloc=np.zeros((K, 8), np.int32))
    names = ["ids", "pword", "dlist", "dcount", "alloc"]
    if opt["staging"]:
        d.update(refinfo=np.zeros((K, 3, B, 2), np.int32), segstart=np.zeros((K, B), np.int32), dseg=np.zeros((K, 2 * B), np.int32),
                 dcnt=np.zeros((K, 2 * B), np.int32), items=np.zeros((K, S, 4), np.int32))
        names += ["refinfo", "segstart", "dseg", "dcnt", "items"]
    out = (ctypes.c_void_p * 10)(*([d[k].ctypes.data for k in names] + [None] * (10 - len(names))))
    _ffi.check(lib.orx_plan_dump(ctx, ptr(u), ptr(p), ptr(n), ptr(labels), K, B, NU, NI, D, o, out, info))
    d.update(item_stride=S, tree_off=np.array([info[1], info[2], info[3]]), index_error=int(info[4]), plan_big=int(info[5]))
    return d


def case_opts(case, version):
    tpw = TPW[case["D"]] if version == 2 and TPW[case["D"]] > 1 and case["B"] >= 2 else 0
    base = dict(version=version, staging=1, urgent=1, tpw=tpw, min_late=-1)
    outs = [base]
    for v in case.get("variants", ()):
        o = dict(base); o.update(v)
        if version == 1:
            o["tpw"] = 0; o["min_late"] = -1
        outs.append(o)
    return outs


def run_case(ctx, case, version):
    u, p, n, lab = make_ids(case)
    NU, NI, D = case["NU"], case["NI"], case["D"]
    geo = geometry(NU, NI, case["B"], n is not None)
    for opt in case_opts(case, version):
        first = None
        for rep in range(2 if version == 2 else 1):
            d = plan_dump(ctx, (u, p, n), lab, NU, NI, D, opt)
            sm = R.check_plan((u, p, n), lab, NU, NI, d, opt, geo)
            if first is not None:
                R.same_unordered(first, sm)
            first = sm


def sequence_opts(step, by):
    """options of one step of a sequence (test_gpu_plan.SEQUENCES): the case's default options of the bucketed plan + the step's overrides"""
    opt = case_opts(by[step["case"]], 2)[0]
    opt.update(step.get("over", {}))
    return opt


def run_sequences(ctx, results):
    from test_gpu_plan import CASES, SEQUENCES
    by = {c["id"]: c for c in CASES}
    for name, steps in SEQUENCES.items():
        t = time.time()
        try:
            for i, step in enumerate(steps):
                case = by[step["case"]]
                u, p, n, lab = make_ids(case)
                geo = geometry(case["NU"], case["NI"], case["B"], n is not None)
                opt = sequence_opts(step, by)
                for _ in range(step.get("repeat", 1)):
                    d = plan_dump(ctx, (u, p, n), lab, case["NU"], case["NI"], case["D"], opt)
                    R.check_plan((u, p, n), lab, case["NU"], case["NI"], d, opt, geo)
                    if "expect_big" in step:
                        assert d["plan_big"] == step["expect_big"], \
                            f"step {i} ({step['case']}): 1024-thread workgroups for the next plan: {d['plan_big']}, expected {step['expect_big']}"
            results[name] = "ok"
        except CASE_ERRORS as e:
            results[name] = f"{type(e).__name__}: {e}"
        results[name + ".seconds"] = round(time.time() - t, 2)
        print(name, results[name], results[name + ".seconds"], flush=True)


def main():
    which, out_path = sys.argv[1], sys.argv[2]
    from openrec_amd import runtime as rt
    from test_gpu_plan import CASES
    ctx = rt.Context(0)
    results = {}
    if which == "seq":
        run_sequences(ctx._h, results)
    else:
        version = 2 if which == "v2" else 1
        for case in CASES:
            t = time.time()
            try:
                run_case(ctx._h, case, version)
                results[case["id"]] = "ok"
            except CASE_ERRORS as e:
                results[case["id"]] = f"{type(e).__name__}: {e}"
            results[case["id"] + ".seconds"] = round(time.time() - t, 2)
            print(case["id"], results[case["id"]], results[case["id"] + ".seconds"], flush=True)
            with open(out_path, "w") as f:
                json.dump(results, f, indent=1)
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
    print(json.dumps(results, indent=1), flush=True)


if __name__ == "__main__":
    main()
