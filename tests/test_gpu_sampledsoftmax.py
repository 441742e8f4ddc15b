"""GPU: the sampled softmax over a shared candidate list (`rt.sampled_softmax_step`, `rt.sampled_softmax_loss`,
`rt.SeqRec.step_sampled` / `loss_sampled`) against tests/sampledsoftmax_ref.py in float64.

Bounds.  A row loss: sampledsoftmax_ref.row_bound, fullsoftmax_ref.row_bound_q on the small table V[[pid_i] + cand].  The loss:
the weighted mean of the row bounds plus (B + 8) u of sum |c_i l_i| for the fp32 sum.  l2: (D + B + 16) u relative, a sum of
B (D + D) squares.  An element of an SGD update: a coefficient a = c pi is exp of a difference of two quantities each within the
row bound e_i, so it is relatively off by at most 2 e_i + (n + 8) u with n the terms of its sum; the reference accumulates
|a| |x| weighted by that (grads(rel=...)), times lr, plus 2 ulp of the element."""
import numpy as np
import pytest

import fullsoftmax_cases as fc
import sampledsoftmax_ref as sr
from conftest import TOL_ADAM, rel_err

pytestmark = pytest.mark.gpu

U32 = sr.U32
NU, NI, LR = 37, 97, 0.05
#          B    S    D
SHAPES = ((1, 1, 8), (1, 200, 64), (1, 63, 256), (63, 63, 20), (63, 65, 256), (63, 200, 64), (65, 1, 20), (65, 65, 64),
          (65, 200, 8), (130, 63, 64), (130, 65, 20), (130, 200, 256))
_CASES = {}


def _rt():
    from openrec_amd import runtime as rt
    return rt


def make(B, S, D, bias=True):
    """the seeded case of a shape, computed once: repeated pids, a candidate that is row 0's own label (and another row's, row 1
    sharing it), a repeated candidate, the label of a middle row as the last candidate, one cand_offset of -inf"""
    key = (B, S, D, bias)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * B + 10 * S + D)
        U, V = (rng.uniform(-fc.SCALE, fc.SCALE, (n, D)).astype(np.float32) for n in (NU, NI))
        b = rng.uniform(-fc.SCALE, fc.SCALE, (NI, 1)).astype(np.float32) if bias else None
        uid, pid, cand = (rng.integers(0, n, m).astype(np.int32) for n, m in ((NU, B), (NI, B), (NI, S)))
        coff, poff = rng.normal(0, 1, S).astype(np.float32), rng.normal(0, 1, B).astype(np.float32)
        w = rng.uniform(0, 2, B).astype(np.float32)
        if B > 1:
            pid[1] = pid[0]
        cand[0] = pid[0]
        if S > 3:
            cand[2], cand[-1], coff[3] = cand[1], pid[B // 2], -np.inf
        _CASES[key] = dict(U=U, V=V, b=b, uid=uid, pid=pid, cand=cand, coff=coff, poff=poff, w=w)
    return _CASES[key]


def _tables(rt, k):
    return tuple(None if x is None else rt.Table(*x.shape).write(x) for x in (k["U"], k["V"], k["b"]))


def _kw(k, **more):
    return dict(weights=k["w"], cand_offset=k["coff"], pos_offset=k["poff"], **more)


def _ref_kw(k, mask_hits=True, scale=1.0):
    return dict(cand_off=k["coff"], pos_off=k["poff"], scale=scale, mask_hits=mask_hits)


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


@pytest.mark.parametrize("mask_hits", [True, False])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-S%d-D%d" % s)
def test_row_losses_loss_and_l2(shape, mask_hits):
    rt, k = _rt(), make(*shape)
    B, S, D = shape
    Q = k["U"][k["uid"]]
    for scale in (1.0, 4.0):
        loss, l2, rows = rt.sampled_softmax_loss(*_tables(rt, k), k["uid"], k["pid"], k["cand"], **_kw(k, scale=scale, mask_hits=mask_hits, per_row=True))
        kw = _ref_kw(k, mask_hits, scale)
        want, bound = sr.row_losses(Q, k["V"], k["b"], k["pid"], k["cand"], **kw), sr.row_bound(Q, k["V"], k["b"], k["pid"], k["cand"], **kw)
        wl, wl2 = sr.forward(Q, k["V"], k["b"], k["pid"], k["cand"], w=k["w"], **kw)
        err = np.abs(rows - want)
        print(f"{shape} mask={mask_hits} scale={scale}: worst row {(err / bound).max():.3g} x bound")
        assert rows.shape == (B,) and (err <= bound).all(), float((err / bound).max())
        c = k["w"].astype(np.float64) / B
        assert abs(loss - wl) <= (c * bound).sum() + (B + 8) * U32 * (c * np.abs(want)).sum() + U32 * abs(wl)
        assert abs(l2 - wl2) <= (D + B + 16) * U32 * wl2


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shape", [(1, 1, 8), (63, 65, 256), (65, 200, 8), (130, 63, 64), (130, 65, 20)], ids=lambda s: "B%d-S%d-D%d" % s)
def test_one_sgd_step_element_by_element(shape, bias):
    rt, k = _rt(), make(*shape, bias=bias)
    B, S, D = shape
    tabs = _tables(rt, k)
    kw = _kw(k, scale=2.0, l2_reg=0.01)
    losses = rt.sampled_softmax_step(rt.Optimizer.sgd(LR), *tabs, k["uid"], k["pid"], k["cand"], **kw)
    assert np.array_equal(_bits(losses[0]), _bits(np.float32(rt.sampled_softmax_loss(*_tables(rt, k), k["uid"], k["pid"], k["cand"],
                                                                                     **_kw(k, scale=2.0))[0])))
    Q, rk = k["U"][k["uid"]], _ref_kw(k, scale=2.0)
    rel = 2 * sr.row_bound(Q, k["V"], k["b"], k["pid"], k["cand"], **rk) + (max(B, S) + 8) * U32
    g = sr.grads(Q, k["V"], k["b"], k["pid"], k["cand"], w=k["w"], l2_reg=float(np.float32(0.01)), rel=rel, **rk)
    checks = [("user", k["U"], tabs[0], k["uid"], g["gq"], g["tq"]), ("item", k["V"], tabs[1], g["rows"], g["gV"], g["tV"])]
    if bias:
        checks.append(("bias", k["b"], tabs[2], g["rows"], g["gb"][:, None], g["tb"][:, None]))
    for name, W0, t, rows, grad, tol in checks:
        got, n = t.read().astype(np.float64), len(W0)
        delta, want = got - W0, -LR * sr.scatter(n, rows, grad)
        cnt = sr.scatter(n, rows, np.ones((len(rows), 1)))
        allowed = LR * sr.scatter(n, rows, tol) + (cnt + 2) * U32 * np.abs(want) + 2 * U32 * np.abs(W0)
        print(f"{shape} {name}: worst element {(np.abs(delta - want) / np.maximum(allowed, 1e-300)).max():.3g} x bound")
        assert (np.abs(delta - want) <= allowed).all(), name
        assert np.array_equal(_bits(t.read())[cnt[:, 0] == 0], _bits(W0)[cnt[:, 0] == 0]), f"{name}: an untouched row changed"
        assert np.abs(delta).max() > 0 or np.abs(want).max() < 1e-9      # (S = 1 with its one candidate masked: no bias gradient)


def test_one_adam_step_leaves_untouched_rows_lazy():
    rt, k = _rt(), make(65, 65, 64)
    tabs, opt, oo = _tables(rt, k), rt.Optimizer.adam(fc.LR["adam"]), fc.make_opt("adam")
    rt.sampled_softmax_step(opt, *tabs, k["uid"], k["pid"], k["cand"], **_kw(k))
    g = sr.grads(k["U"][k["uid"]], k["V"], k["b"], k["pid"], k["cand"], w=k["w"], **_ref_kw(k))
    V, b = k["V"].astype(np.float64), k["b"].astype(np.float64)
    oo.begin_step()
    oo.apply(V, g["rows"], g["gV"], key="V"); oo.apply(b, g["rows"], g["gb"][:, None], key="b")
    idle = np.setdiff1d(np.arange(NI), g["rows"])
    assert len(idle) > 5
    for t, W0, want in ((tabs[1], k["V"], V), (tabs[2], k["b"], b)):
        assert rel_err(t.read(), want.astype(np.float32)) <= TOL_ADAM
        assert np.array_equal(_bits(t.read())[idle], _bits(W0)[idle])
        for slot in (0, 1):
            assert not _bits(np.asarray(opt.slot(t, slot)).reshape(W0.shape))[idle].any()


def test_bag_form_equals_the_user_table_form_and_runs_repeat():
    rt, k = _rt(), make(130, 65, 20)
    ptr, items = fc.make_bags(dict(seed=5, B=130, NI=NI))
    res = []
    for form in ("bags", "bags", "table"):
        H, V, b = _tables(rt, dict(k, U=k["V"][::-1].copy()))
        net, opt = rt.SeqRec(H, V, b), rt.Optimizer.sgd(LR)
        if form == "bags":
            fwd = net.loss_sampled((ptr, items), k["pid"], k["cand"], **_kw(k))
            losses = net.step_sampled(opt, (ptr, items), k["pid"], k["cand"], **_kw(k, l2_reg=0.01))
        else:
            Q = net.user_table((ptr, items))
            uid = np.arange(130, dtype=np.int32)
            fwd = rt.sampled_softmax_loss(Q, V, b, uid, k["pid"], k["cand"], **_kw(k))
            losses = rt.sampled_softmax_step(opt, Q, V, b, uid, k["pid"], k["cand"], **_kw(k, l2_reg=0.01))
        assert np.array_equal(_bits(np.float32(fwd)), _bits(np.concatenate(losses)))      # the forward is the step's loss and l2
        res.append([_bits(V.read()), _bits(b.read()), _bits(np.concatenate(losses)), _bits(H.read())])
    assert all(np.array_equal(x, y) for x, y in zip(res[0], res[1]))                      # two runs, identical bits
    assert all(np.array_equal(x, y) for x, y in zip(res[0][:3], res[2][:3]))              # the item side, bit for bit
    assert not np.array_equal(res[0][0], _bits(k["V"]))


@pytest.mark.parametrize("edge", ["bad_cand", "bad_pid", "all_removed", "no_candidates", "train_user"])
def test_edges_leave_the_context_usable(edge):
    rt, k = _rt(), dict(make(65, 65, 64))
    B, live, train = 65, np.ones(65, bool), None
    if edge == "bad_cand":
        k["cand"] = k["cand"].copy(); k["cand"][5] = NI + 3
    elif edge == "bad_pid":
        k["pid"] = k["pid"].copy(); k["pid"][7] = -2; live[7] = False
    elif edge == "all_removed":
        k["coff"] = np.full(65, -np.inf, np.float32)
    elif edge == "no_candidates":
        k["cand"], k["coff"] = k["cand"][:0], k["coff"][:0]
    else:
        train = ("user",)
    tabs, kw = _tables(rt, k), _kw(k)
    before = [_bits(t.read()) for t in tabs]
    step = lambda: rt.sampled_softmax_step(rt.Optimizer.sgd(LR), *tabs, k["uid"], k["pid"], k["cand"], l2_reg=0.0, train=train, **kw)
    if edge in ("bad_cand", "bad_pid"):
        with pytest.raises(IndexError):                     # reported, and what is live has been applied: the bad column / sample is ignored
            step()
        g = sr.grads(k["U"][k["uid"]], k["V"], k["b"], np.where(live, k["pid"], 0), k["cand"], w=k["w"], live=live, **_ref_kw(k))
        want = k["V"] - LR * sr.scatter(NI, g["rows"], g["gV"])
        assert rel_err(tabs[1].read(), want) <= 1e-5
        k = make(65, 65, 64)                                # the context is usable: the clean case on it is right
        tabs, kw = _tables(rt, k), _kw(k)
    loss, l2, rows = rt.sampled_softmax_loss(*tabs, k["uid"], k["pid"], k["cand"], per_row=True, **kw)
    Q = k["U"][k["uid"]]
    want = sr.row_losses(Q, k["V"], k["b"], k["pid"], k["cand"], **_ref_kw(k))
    assert (np.abs(rows - want) <= sr.row_bound(Q, k["V"], k["b"], k["pid"], k["cand"], **_ref_kw(k))).all()
    if edge in ("all_removed", "no_candidates"):
        assert not rows.any() and loss == 0.0
        step()
        assert all(np.array_equal(x, _bits(t.read())) for x, t in zip(before, tabs))       # l_i = 0 and l2_reg = 0: no gradient at all
    if edge == "train_user":
        step()
        after = [_bits(t.read()) for t in tabs]
        assert np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2]) and not np.array_equal(before[0], after[0])
