"""What the CG ALS tests share, on the shapes of tests/als_cases.py (tests/test_als_cg_cpu.py proves each bound meaningful on the
CPU, tests/test_gpu_als_cg.py holds the device to it).  A solved half carries x64 = cg64, x32 = cg32 (the float32 yardstick) and
e32cg = max|x32 - x64| / max|x64| of the SAME case and step count; the device's bound is FACTOR_CG e32cg.

FACTOR_CG: at up to 3 steps a second float32 ordering of the same sums (als_cg_ref.cg32_permuted) lands up to 3.7 e32cg from cg64;
the factor is that spread doubled and rounded up to a power of two.  The bound is for FEW steps only: an unconverged CG amplifies
rounding on the ill-conditioned cases (at 10 steps cg32 and cg64 are 0.1 - 0.4 apart where reg = 0.1), so there is no element-wise
bound there.  References are computed once per process and never modified."""
import functools

import numpy as np

import als_cases as ac
import als_cg_ref as cr
import als_ref as ar

FACTOR_CG = 8.0
CG_STEPS = (1, 2, 3)
HALVES = [("acc", k, side) for k in range(len(ac.ACC_CASES)) for side in ("user", "item")] + [("conf",)]


def half_id(which):
    return "per-entry-conf" if which[0] == "conf" else f"{ac.case_id(ac.ACC_CASES[which[1]])}-{which[2]}"


def half(which):
    """the half-step of tests/als_cases.py named by an element of HALVES"""
    return ac.accuracy_case(which[1])[which[2]] if which[0] == "acc" else ac.conf_case()


def _args(h):
    return h["F"], h["X0"], h["ptr"], h["cols"], h["conf"], h["a"], h["b"], h["reg"]


def solve(h, steps):
    x64, x32 = cr.cg64(*_args(h), steps), cr.cg32(*_args(h), steps)
    out = dict(h)
    out.update(x64=x64, x32=x32, e32cg=ar.err_vs(x32, x64), steps=steps)
    return out


@functools.lru_cache(maxsize=None)
def solved(which, steps):
    """-> the half with x64 / x32 / e32cg of `steps` CG steps from its X0"""
    return solve(half(which), steps)


# "it is CG": the well-conditioned halves at D = 8, where 16 steps are the direct solution
CONVERGED_STEPS = 16
CONVERGED = [("acc", k, side) for k, c in enumerate(ac.ACC_CASES) if c["D"] == 8 and c["reg"] == 10.0 for side in ("user", "item")]


@functools.lru_cache(maxsize=None)
def converged(which):
    """-> the half, x32 = cg32 after CONVERGED_STEPS steps and `bound` = max(err_vs(x32, the direct float64 solution), e32)"""
    h = half(which)
    x32 = cr.cg32(*_args(h), CONVERGED_STEPS)
    return dict(h, x32cg=x32, bound=max(ar.err_vs(x32, h["x64"]), h["e32"]))


@functools.lru_cache(maxsize=None)
def breaks_case(breaks, L, steps=3):
    """the rows of als_cases.long_case(L) and, for every t of `breaks`, rows of t - 1, t and t + 1 observations, solved"""
    base = ac.long_case(L)
    M, D = base["F"].shape
    rng = np.random.default_rng(92)
    counts = [n for t in breaks for n in (t - 1, t, t + 1)]
    rows = [np.sort(rng.choice(M, n, replace=False)).astype(np.int32) for n in counts]
    ptr = np.concatenate([base["ptr"], base["ptr"][-1] + np.cumsum(counts)]).astype(np.int64)
    cols = np.concatenate([base["cols"]] + rows).astype(np.int32)
    X0 = np.concatenate([base["X0"], rng.uniform(-0.5, 0.5, (len(counts), D)).astype(np.float32)])
    h = dict(F=base["F"], X0=X0, ptr=ptr, cols=cols, conf=None, a=base["a"], b=base["b"], reg=base["reg"])
    return solve(h, steps)


DESCENT = dict(a=41.0, b=1.0, reg=0.1, D=64, seed=4, sweeps=3)


def descent_reference(steps, dtype):
    """the objective (dense, float64) before and after every half-step of DESCENT["sweeps"] sweeps of the reference"""
    d = DESCENT
    rec = ac.interactions()
    pu, cu = ac.csr_of(rec, ac.NU, ac.NI)
    pi, ci = ac.csr_of(rec, ac.NI, ac.NU, "item_id", "user_id")
    C, P = ar.dense_conf(pu, cu, None, d["a"], d["b"], (ac.NU, ac.NI))
    U, V = (x.astype(dtype) for x in ac.tables(d["D"], d["seed"]))
    cg = cr.cg64 if dtype == np.float64 else cr.cg32
    obj = [ar.objective(U, V, C, P, d["reg"])]
    for _ in range(d["sweeps"]):
        U = cg(V, U, pu, cu, None, d["a"], d["b"], d["reg"], steps); obj.append(ar.objective(U, V, C, P, d["reg"]))
        V = cg(U, V, pi, ci, None, d["a"], d["b"], d["reg"], steps); obj.append(ar.objective(U, V, C, P, d["reg"]))
    return obj


TOY_CG_STEPS = 3
TOY_CG_SWEEPS = 2                  # tests/test_als_cg_cpu.py: cg64 ranks the held items first after this many sweeps


def toy_reference(sweeps, steps=TOY_CG_STEPS):
    """the toy set of als_cases trained by cg64 -> (scores with the training items at -inf, held lists, user -> items CSR)"""
    t = ac.TOY
    rec, held = ac.toy_set()
    nu, ni = t["groups"] * t["users_per"], t["groups"] * t["items_per"]
    pu, cu = ac.csr_of(rec, nu, ni)
    pi, ci = ac.csr_of(rec, ni, nu, "item_id", "user_id")
    U, V = (x.astype(np.float64) for x in ac.toy_init())
    for _ in range(sweeps):
        U = cr.cg64(V, U, pu, cu, None, t["a"], t["b"], t["reg"], steps)
        V = cr.cg64(U, V, pi, ci, None, t["a"], t["b"], t["reg"], steps)
    S = U @ V.T
    for u in range(nu):
        S[u, cu[pu[u]:pu[u + 1]]] = -np.inf
    return S, held, (pu, cu)


def objective_cases():
    """(name, U, V, ptr, cols, conf, a, b, reg): the interactions() set at D = 8, 64 and 128, and the per-entry-confidence case"""
    rec = ac.interactions()
    pu, cu = ac.csr_of(rec, ac.NU, ac.NI)
    out = []
    for D in (8, 64, 128):
        U, V = ac.tables(D, 300 + D)
        out.append((f"interactions-D{D}", U, V, pu, cu, None, DESCENT["a"], DESCENT["b"], DESCENT["reg"]))
    h = ac.conf_case()
    out.append(("per-entry-conf", h["X0"], h["F"], h["ptr"], h["cols"], h["conf"], h["a"], h["b"], h["reg"]))
    return out
