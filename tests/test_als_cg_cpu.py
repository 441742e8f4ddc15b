"""CPU: the CG ALS reference (tests/als_cg_ref.py) is conjugate gradient on the half-step's system and a descent method of its
objective, and every bound tests/test_gpu_als_cg.py holds the device to is a real bound before any GPU sees it: the float32
yardstick error e32cg is non-zero and finite on every case, a second float32 ordering stays within FACTOR_CG of it, and the
objective's rounding bound is small against the objective."""
import numpy as np
import pytest

import als_cases as ac
import als_cg_cases as cc
import als_cg_ref as cr
import als_ref as ar


@pytest.mark.parametrize("which", cc.HALVES, ids=cc.half_id)
def test_yardstick_error_and_a_second_float32_ordering(which):
    for steps in cc.CG_STEPS:
        h = cc.solved(which, steps)
        xp = cr.cg32_permuted(*cc._args(h), steps)
        ep = ar.err_vs(xp, h["x64"])
        print(f"steps {steps}: e32cg = {h['e32cg']:.3g}, permuted ordering {ep:.3g}, ratio {ep / h['e32cg']:.3g}")
        assert np.isfinite(h["x64"]).all() and np.isfinite(h["x32"]).all()
        assert np.isfinite(h["e32cg"]) and 0.0 < h["e32cg"] < 1e-3
        assert h["x32"].dtype == np.float32 and h["x64"].dtype == np.float64
        assert ep <= cc.FACTOR_CG * h["e32cg"]
        assert not h["x64"][0].any() and not h["x32"][0].any()        # the row without observations


@pytest.mark.parametrize("D", [8, 50])
def test_2d_steps_are_the_direct_solution(D):
    """it is CG: in float64, 2 D steps reproduce the closed form of als_ref.half_step to 1e-6 relative"""
    k = next(i for i, c in enumerate(ac.ACC_CASES) if c["D"] == D and c["a"] == 41.0 and c["reg"] == 0.1)
    for side, h in ac.accuracy_case(k).items():
        err = ar.err_vs(cr.cg64(*cc._args(h), 2 * D), h["x64"])
        print(f"D {D} {side}: {err:.3g}")
        assert err <= 1e-6


@pytest.mark.parametrize("which", cc.CONVERGED, ids=cc.half_id)
def test_converged_yardstick_is_close_to_the_direct_solution(which):
    """the bound of the GPU's converged test means something: the float32 CG sits within 1e-4 of the direct float64 solution"""
    c = cc.converged(which)
    print(f"bound {c['bound']:.3g} (e32 of the direct solve {c['e32']:.3g})")
    assert 0.0 < c["bound"] < 1e-4


def test_warm_start_matters():
    """one step from two different starts gives different rows (the GPU test asks the same of the device)"""
    h = cc.solved(cc.HALVES[0], 1)
    other = cr.cg64(h["F"], -h["X0"], h["ptr"], h["cols"], h["conf"], h["a"], h["b"], h["reg"], 1)
    assert np.abs(other[1:] - h["x64"][1:]).max() > 1e-3


def test_zero_residual_freezes_the_row():
    """y = 0 and x = 0: r = 0, and the guard keeps 0 / 0 out of x"""
    h = dict(cc.half(cc.HALVES[0]))
    conf = np.zeros(h["cols"].size, np.float32)
    for f in (cr.cg64, cr.cg32):
        x = f(h["F"], np.zeros_like(h["X0"]), h["ptr"], h["cols"], conf, 1.0, 0.0, h["reg"], 3)
        assert np.isfinite(x).all() and not x.any()


@pytest.mark.parametrize("steps, last", [(1, 494.3), (3, 61.96)])
def test_reference_descends(steps, last):
    for dtype in (np.float32, np.float64):
        obj = cc.descent_reference(steps, dtype)
        print(dtype.__name__, ["%.6g" % o for o in obj])
        for o0, o1 in zip(obj, obj[1:]):
            assert o1 <= o0 + 1e-5 * abs(o0)
        assert obj[-1] < 0.5 * obj[0]
        assert abs(obj[0] - 18719.5) < 0.1 and abs(obj[-1] - last) <= 2e-3 * last


def test_toy_set_needs_this_many_sweeps():
    """cg64 with TOY_CG_STEPS steps ranks the held items first after TOY_CG_SWEEPS sweeps (no more than the closed form's 2),
    the last held item leading the first other one by far more than fp32 can move a score"""
    assert cc.TOY_CG_SWEEPS >= ac.TOY["sweeps"]
    S, held, _ = cc.toy_reference(cc.TOY_CG_SWEEPS)
    n = ac.TOY["held"]
    for u in range(S.shape[0]):
        order = np.argsort(-S[u])
        assert np.array_equal(np.sort(order[:n]), held[u]), (u, order[:n], held[u])
        assert S[u, order[n - 1]] - S[u, order[n]] > 1e-3


@pytest.mark.parametrize("case", cc.objective_cases(), ids=lambda c: c[0])
def test_objective_sparse_form_and_its_bound(case):
    name, U, V, ptr, cols, conf, a, b, reg = case
    C, P = ar.dense_conf(ptr, cols, conf, a, b, (U.shape[0], V.shape[0]))
    dense = ar.objective(U, V, C, P, reg)
    o64, o32 = cr.objective64(U, V, ptr, cols, conf, a, b, reg), cr.objective32(U, V, ptr, cols, conf, a, b, reg)
    bound = cr.objective_bound(U, V, ptr, cols, conf, a, b, reg)
    print(f"{name}: dense {dense:.12g}, sparse64 off by {abs(o64 - dense):.3g}, sparse32 off by {abs(o32 - dense):.3g}, bound {bound:.3g}")
    assert abs(o64 - dense) <= 1e-12 * dense                  # the formula is the objective
    assert 0.0 < abs(o32 - dense) <= bound                    # float32 rounding is visible and within the bound
    assert bound < 1e-3 * dense
