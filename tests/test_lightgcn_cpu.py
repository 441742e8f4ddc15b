"""CPU: the references of tests/lightgcn_ref.py agree with each other, the exact cases are exact in float32 in any order, the
tolerance bound holds for a float32 evaluation, and the wrappers refuse bad arguments before the library is called."""
import numpy as np
import pytest

import lightgcn_cases as lc
import lightgcn_ref as lr

def _segment_len():
    from openrec_amd import runtime as rt
    return rt.graph_segment_len()


def test_csr_and_dense_references_agree():
    s = lc.step_setup()
    uid, pid, nid = lc.step_batches()[0]
    fu, fv = lr.propagate(s["U"], s["V"], s["by_user"], s["by_item"], s["su"], s["sv"], s["al"])
    du, dv = lr.propagate_dense(s["A"], s["U"], s["V"], s["al"])
    assert np.abs(fu - du).max() <= 1e-12 and np.abs(fv - dv).max() <= 1e-12
    for l2 in (0.0, 0.01):
        a = lr.grads_csr(s["U"], s["V"], s["by_user"], s["by_item"], s["su"], s["sv"], s["al"], uid, pid, nid, l2)
        b = lr.loss_dense(s["A"], s["U"], s["V"], s["al"], uid, pid, nid, l2)
        assert abs(a[0] - b[0]) <= 1e-12 and abs(a[1] - b[1]) <= 1e-12
        assert np.abs(a[2] - b[2]).max() <= 1e-12 and np.abs(a[3] - b[3]).max() <= 1e-12, "backward is not forward"
        assert np.abs(b[2]).max() > 1e-4
    assert s["A"].shape == (500, 500) and np.array_equal(s["A"], s["A"].T)


def _exact(U, V, by_user, by_item, su, sv, al):
    f64 = lr.propagate(U, V, by_user, by_item, su, sv, al)
    for rev in (False, True):
        f32 = lr.propagate(U, V, by_user, by_item, su, sv, al, np.float32, reverse=rev)
        for a, b in zip(f32, f64):
            assert a.dtype == np.float32 and np.array_equal(a.astype(np.float64), b), "float32 is not exact on this case"
    return f64


def test_long_row_case_is_exact_in_float32_in_any_order():
    S = _segment_len()
    by_user, by_item = lc.long_graph(S)
    U, V = lc.int_tables(lc.LONG_NU, lc.LONG_NI, 16, 1)
    fu, fv = _exact(U, V, by_user, by_item, lr.unit(lc.LONG_NU), lr.unit(lc.LONG_NI), np.ones(3, np.float32))
    assert max(np.abs(fu).max(), np.abs(fv).max()) < 2 ** 24
    for D in (1, 50, 64, 100, 128):
        U, V = lc.int_tables(lc.LONG_NU, lc.LONG_NI, D, 10 + D)
        _exact(U, V, by_user, by_item, lr.unit(lc.LONG_NU), lr.unit(lc.LONG_NI), np.ones(2, np.float32))


def test_biregular_case_is_exact_in_float32():
    by_user, by_item = lc.biregular()
    su, sv = lr.scales(by_user[0]), lr.scales(by_item[0])
    assert set(su) == {np.float32(0.5)} and set(sv) == {np.float32(0.25)}
    for D in (16, 50):
        U, V = lc.int_tables(64, 16, D, 20 + D)
        _exact(U, V, by_user, by_item, su, sv, lc.default_weights(3))


@pytest.mark.parametrize("D,L", lc.GEN_CASES)
def test_bound_holds_for_float32_in_two_orders(D, L):
    h = lc.general_case(D, L)
    assert h["n_max"] >= 100
    worst = 0.0
    for rev in (False, True):
        f32 = lr.propagate(h["U"], h["V"], h["by_user"], h["by_item"], h["su"], h["sv"], h["al"], np.float32, reverse=rev)
        for got, ref, bd in ((f32[0], h["fu"], h["bu"]), (f32[1], h["fv"], h["bv"])):
            err = np.abs(got.astype(np.float64) - ref)
            assert (err <= bd).all()
            live = bd > 0
            worst = max(worst, float((err[live] / bd[live]).max()))
    print(f"D {D} L {L}: n_max {h['n_max']}, float32 uses at most {worst:.3g} of the bound")
    assert 0 < worst < 0.05
    # a row with no path: the bound is alpha_0 |E(0)| L (n + 8) u there, and the value alpha_0 E(0) exactly
    assert np.array_equal(h["fu"][lc.GEN_EMPTY_USER], np.float64(h["al"][0]) * h["U"][lc.GEN_EMPTY_USER])


def test_topk_case_is_separated():
    h = lc.topk_case()
    assert h["users"].size >= h["nu"] // 2, "too few users whose k-th and (k+1)-th scores are far apart"
    assert (h["gap"][h["users"]] > 200 * h["score_bound"]).all()


def test_scales_are_numpy_float32():
    ptr = np.array([0, 0, 1, 4, 13], np.int64)
    s = lr.scales(ptr)
    assert s.dtype == np.float32 and s[0] == 0 and s[1] == 1 and s[3] == np.float32(1) / np.sqrt(np.float32(9))
    from openrec_amd import runtime as rt
    csr = rt.ALSCsr(ptr, np.arange(13, dtype=np.int32), None, 13)
    assert np.array_equal(rt.graph_scales(csr).view(np.int32), s.view(np.int32))


# ---- argument checks that need no device -------------------------------------------------------------------------------------
class _T:
    """a stand-in table: the wrappers' checks read these fields only"""
    class _H:
        def __init__(self, v): self.value = v

    def __init__(self, rows, dim, ctx="ctx", h=None):
        self.rows, self.dim, self.ctx = rows, dim, ctx
        self._h = _T._H(h if h is not None else id(self))


def _rt():
    from openrec_amd import runtime as rt
    return rt


def test_graph_spmm_argument_checks():
    rt = _rt()
    csr = rt.ALSCsr(np.array([0, 1, 2], np.int64), np.array([0, 2], np.int32), None, 3)
    X, out, acc = _T(3, 8), _T(2, 8), _T(2, 8)
    with pytest.raises(ValueError, match="same table"):
        rt.graph_spmm(X, X, csr)
    with pytest.raises(ValueError, match="same table"):
        rt.graph_spmm(X, out, csr, acc=X)
    with pytest.raises(ValueError, match="dim"):
        rt.graph_spmm(X, _T(2, 4), csr)
    with pytest.raises(ValueError, match="different contexts"):
        rt.graph_spmm(X, _T(2, 8, ctx="other"), csr)
    with pytest.raises(ValueError, match="outside"):
        rt.graph_spmm(_T(3, 129), _T(2, 129), csr)
    with pytest.raises(ValueError, match="shape"):
        rt.graph_spmm(_T(4, 8), out, csr)
    with pytest.raises(ValueError, match="rows"):
        rt.graph_spmm(X, out, csr, rows=(1, 2))
    with pytest.raises(ValueError, match="acc has"):
        rt.graph_spmm(X, out, csr, acc=_T(3, 8))
    with pytest.raises(ValueError, match="ALSCsr"):
        rt.graph_spmm(X, out, (csr.ptr, csr.cols))
    with pytest.raises(ValueError, match="norm"):
        rt.InteractionGraph(None, 1, 1, norm="left")


def test_lightgcn_argument_checks():
    rt = _rt()
    g = rt.InteractionGraph.__new__(rt.InteractionGraph)
    g.ctx, g.total_users, g.total_items = "ctx", 5, 7
    U, V = _T(5, 8), _T(7, 8)
    for layers in (0, 9):
        with pytest.raises(ValueError, match="layers"):
            rt.LightGCN(U, V, g, layers=layers)
    with pytest.raises(ValueError, match="layer weights"):
        rt.LightGCN(U, V, g, layers=2, layer_weights=(1, 1))
    with pytest.raises(ValueError, match="graph of"):
        rt.LightGCN(_T(6, 8), V, g)
    with pytest.raises(ValueError, match="contexts"):
        rt.LightGCN(_T(5, 8, ctx="other"), V, g)
    with pytest.raises(ValueError, match="outside"):
        rt.LightGCN(_T(5, 129), _T(7, 129), g)
    with pytest.raises(ValueError, match="dim"):
        rt.LightGCN(U, _T(7, 4), g)
    with pytest.raises(ValueError, match="bias"):
        rt.LightGCN(U, V, g, bias=_T(7, 1))
    with pytest.raises(ValueError, match="InteractionGraph"):
        rt.LightGCN(U, V, "graph")
    with pytest.raises(ValueError, match="same table"):
        rt.LightGCN(U, U, g)
