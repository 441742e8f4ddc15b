"""CPU: the ALS reference (tests/als_ref.py) is a minimiser and a descent method, and every shared case (tests/als_cases.py) has a
float32 yardstick error that is non-zero and finite -- so `4 e32`, the bound tests/test_gpu_als.py holds the device to, is a real
bound before any GPU sees it."""
import numpy as np
import pytest

import als_cases as ac
import als_ref as ar


def _halves():
    for k, c in enumerate(ac.ACC_CASES):
        for side in ("user", "item"):
            yield pytest.param(("acc", k, side), id=f"{ac.case_id(c)}-{side}")
    yield pytest.param(("conf",), id="per-entry-conf")
    yield pytest.param(("long",), id="long-rows")


def _half(which):
    if which[0] == "acc":
        return ac.accuracy_case(which[1])[which[2]]
    if which[0] == "conf":
        return ac.conf_case()
    from openrec_amd import runtime as rt
    return ac.long_case(rt.als_segment_len())


@pytest.mark.parametrize("which", list(_halves()))
def test_yardstick_error_is_nonzero_and_finite(which):
    h = _half(which)
    print(f"e32 = {h['e32']:.3g}")
    assert np.isfinite(h["x64"]).all() and np.isfinite(h["x32"]).all()
    assert np.isfinite(h["e32"]) and 0.0 < h["e32"] < 1e-2
    assert h["x32"].dtype == np.float32 and h["x64"].dtype == np.float64


@pytest.mark.parametrize("k", [0, 3, 12, 21, 30], ids=lambda k: ac.case_id(ac.ACC_CASES[k]))
def test_half_step_zeroes_the_gradient(k):
    """the reference half-step is the exact minimiser in X: the objective's gradient with respect to X vanishes to 1e-9 of the
    gradient's size before the step"""
    for side, h in ac.accuracy_case(k).items():
        C, P = ar.dense_conf(h["ptr"], h["cols"], h["conf"], h["a"], h["b"], (h["X0"].shape[0], h["F"].shape[0]))
        g0 = ar.gradient_X(h["F"], h["X0"], C, P, h["reg"])
        g1 = ar.gradient_X(h["F"], h["x64"], C, P, h["reg"])
        print(f"{side}: |grad| before {np.abs(g0).max():.3g}, after {np.abs(g1).max():.3g}")
        assert np.abs(g1).max() <= 1e-9 * np.abs(g0).max()
        assert not h["x64"][0].any()                  # the row without observations


def test_conf_case_gradient_and_merge():
    h = ac.conf_case()
    C, P = ar.dense_conf(h["ptr"], h["cols"], h["conf"], h["a"], h["b"], (ac.NU, ac.NI))
    g0 = ar.gradient_X(h["F"], h["X0"], C, P, h["reg"])
    g1 = ar.gradient_X(h["F"], h["x64"], C, P, h["reg"])
    assert np.abs(g1).max() <= 1e-9 * np.abs(g0).max()
    assert (h["conf"] == ac.CONF_B).sum() >= h["cols"].size // 4          # zero-weight updates are in the case
    # the records really hold duplicates, and merged by hand they are the case's CSR
    ptr, cols = ac.csr_of(h["records"], ac.NU, ac.NI)
    assert h["records"].size > cols.size
    assert np.array_equal(ptr, h["ptr"]) and np.array_equal(cols, h["cols"])


@pytest.mark.parametrize("ab", ac.ABS, ids=lambda ab: "a%g-b%g" % ab)
def test_sweeps_never_increase_the_objective(ab):
    a, b = ab
    rec = ac.interactions()
    pu, cu = ac.csr_of(rec, ac.NU, ac.NI)
    pi, ci = ac.csr_of(rec, ac.NI, ac.NU, "item_id", "user_id")
    C, P = ar.dense_conf(pu, cu, None, a, b, (ac.NU, ac.NI))
    U, V = (x.astype(np.float64) for x in ac.tables(16, 3))
    obj = [ar.objective(U, V, C, P, 0.1)]
    for _ in range(3):
        U = ar.half_step(V, U, pu, cu, None, a, b, 0.1); obj.append(ar.objective(U, V, C, P, 0.1))
        V = ar.half_step(U, V, pi, ci, None, a, b, 0.1); obj.append(ar.objective(U, V, C, P, 0.1))
    print(["%.6g" % o for o in obj])
    for o0, o1 in zip(obj, obj[1:]):
        assert o1 <= o0 * (1 + 1e-12)
    assert obj[-1] < obj[0]


def test_descent_slack_of_fp32_tables():
    """what rounding the tables to float32 after every half-step (the device keeps them in fp32) can add to the objective: far
    below the 1e-5 |objective| the GPU descent test allows"""
    a, b = 41.0, 1.0
    rec = ac.interactions()
    pu, cu = ac.csr_of(rec, ac.NU, ac.NI)
    C, P = ar.dense_conf(pu, cu, None, a, b, (ac.NU, ac.NI))
    U, V = ac.tables(64, 4)
    U64 = ar.half_step(V, U, pu, cu, None, a, b, 0.1)
    o64, o32 = ar.objective(U64, V, C, P, 0.1), ar.objective(U64.astype(np.float32), V, C, P, 0.1)
    print(f"objective {o64:.9g}, with the solution rounded to fp32 {o32:.9g}, relative {abs(o32 - o64) / o64:.3g}")
    assert abs(o32 - o64) <= 1e-7 * o64


def test_toy_set_ranks_held_items_first_for_the_reference():
    """the block-diagonal toy set of the class test does what the GPU test asks of it when trained by the float64 reference"""
    t = ac.TOY
    rec, held = ac.toy_set()
    nu, ni = t["groups"] * t["users_per"], t["groups"] * t["items_per"]
    pu, cu = ac.csr_of(rec, nu, ni)
    pi, ci = ac.csr_of(rec, ni, nu, "item_id", "user_id")
    U, V = (x.astype(np.float64) for x in ac.toy_init())
    for _ in range(t["sweeps"]):
        U = ar.half_step(V, U, pu, cu, None, t["a"], t["b"], t["reg"])
        V = ar.half_step(U, V, pi, ci, None, t["a"], t["b"], t["reg"])
    S = U @ V.T
    for u in range(nu):
        S[u, cu[pu[u]:pu[u + 1]]] = -np.inf
        order = np.argsort(-S[u])
        assert np.array_equal(np.sort(order[:t["held"]]), held[u]), (u, order[:t["held"]], held[u])
        # the last held item leads the first other item by far more than fp32 can move a score
        assert S[u, order[t["held"] - 1]] - S[u, order[t["held"]]] > 1e-3
