"""GPU: the full softmax with bf16 operands on the matrix cores (precision="bf16", ORX_FS_BF16) against the rounded semantics of
include/openrec_hip.h in float64: bf(x) is a torch.bfloat16 round trip, every sum is float64.

Row losses are held to fullsoftmax_ref.row_bound on the bf16-rounded tables.  Products of bf16 values are exact in fp32 and the
instruction sums them in fp32, so the fp32 path's bound holds as it stands: the worst row measured over the seven shapes is
0.024 of it.  A gradient element is held to (2^-8 + TOL) * scale * sum |a*| |bf(x)| + TOL |l2 term| + 2 ulp(W): 2^-9 is the
coefficient's bf16 rounding, doubled for the device's own a; TOL is fp32 accumulation; the ulp term is delta_check's."""
import numpy as np
import pytest
import torch

import fullsoftmax_cases as fc
import fullsoftmax_ref as fr
from conftest import TOL, delta_check

pytestmark = pytest.mark.gpu


def _rt():
    from openrec_amd import runtime as rt
    return rt


def bf(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, np.float32)).bfloat16().float().numpy()


def _f64(x):
    return None if x is None else np.asarray(x, np.float64)


def _tables(rt, *arrays):
    return tuple(None if x is None else rt.Table(*x.shape).write(x) for x in arrays)


def ref_grads(U, V, b, uid, pid, w, off, scale, l2_reg):
    """the rounded semantics in float64 -> (loss, l2_loss, {name: (gradient, its bound without the ulp term)}) for U[uid] rows, V, b"""
    Q, Qb, Vb, V64, b64 = _f64(U)[uid], _f64(bf(U))[uid], _f64(bf(V)), _f64(V), _f64(b)
    loss, _ = fr.forward_q(Qb, Vb, b64, pid, _f64(w), _f64(off), scale)
    l2 = 0.5 * ((Q * Q).sum() + (V64[pid] ** 2).sum())
    a, _ = fr.coefficients(Qb, Vb, b64, pid, _f64(w), _f64(off), scale)
    ab = _f64(bf(a))
    n = np.bincount(pid, minlength=len(V)).astype(np.float64)
    lq, lv = l2_reg * Q, (l2_reg * n)[:, None] * V64
    k = 2.0 ** -8 + TOL
    return loss, l2, dict(gu=(scale * ab @ Vb + lq, k * scale * np.abs(a) @ np.abs(Vb) + TOL * np.abs(lq)),
                          GV=(scale * ab.T @ Qb + lv, k * scale * np.abs(a).T @ np.abs(Qb) + TOL * np.abs(lv)),
                          Gb=(scale * a.sum(0), None))


# ---- 1. row losses ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(1, len(fc.SHAPES)))
def test_every_row_loss_is_within_the_bound_of_the_rounded_tables(si):
    rt = _rt()
    case = fc.shape_case(si, seed=500 + si)
    U, V, b, uid, pid = fc.make(case)
    off = np.random.default_rng(21 + si).normal(0, 1, case["NI"]).astype(np.float32)
    tabs = _tables(rt, U, V, b)
    for scale in (1.0, 4.0):
        loss, l2, rows = rt.fullsoftmax_loss(*tabs, uid, pid, item_offset=off, scale=scale, chunk_items=case["chunk_items"], per_row=True,
                                             precision="bf16")
        want = fr.row_losses(_f64(bf(U)), _f64(bf(V)), _f64(b), uid, pid, _f64(off), scale)
        bound = fr.row_bound(bf(U), bf(V), b, uid, pid, off, scale)
        err = np.abs(rows.astype(np.float64) - want)
        print(f"{case['name']} scale={scale}: worst row {(err / bound).max():.3g} x bound")
        assert rows.shape == (case["B"],) and (err <= bound).all(), float((err / bound).max())
        assert abs(loss - want.mean()) <= TOL * abs(want.mean())


# ---- 2. the rounding is where the semantics put it ----------------------------------------------------------------------------------
@pytest.mark.parametrize("si", [2, 3])
def test_the_rows_are_those_of_the_rounded_tables_and_not_of_the_fp32_tables(si):
    rt = _rt()
    case = fc.shape_case(si, seed=500 + si)
    U, V, b, uid, pid = fc.make(case)
    rows = rt.fullsoftmax_loss(*_tables(rt, U, V, b), uid, pid, per_row=True, precision="bf16")[2].astype(np.float64)
    inside = np.abs(rows - fr.row_losses(_f64(bf(U)), _f64(bf(V)), _f64(b), uid, pid)) <= fr.row_bound(bf(U), bf(V), b, uid, pid)
    outside = np.abs(rows - fr.row_losses(_f64(U), _f64(V), _f64(b), uid, pid)) > fr.row_bound(U, V, b, uid, pid)
    print(f"{case['name']}: {outside.mean():.2f} of the rows outside the bound of the unrounded tables")
    assert inside.all() and outside.mean() > 0.5


# ---- 3. one SGD step with lr = 1: W0 - W1 is the gradient ---------------------------------------------------------------------------
@pytest.mark.parametrize("si,bias,extras,device", [(1, True, False, False), (3, False, False, True), (4, True, True, False), (6, False, False, False),
                                                   (3, True, False, False), (6, True, False, True)])
def test_one_sgd_step_gives_the_gradients_of_the_rounded_semantics(si, bias, extras, device):
    rt = _rt()
    case = fc.shape_case(si, bias=bias, seed=900 + si)
    U, V, b, uid, pid = fc.make(case)
    rng = np.random.default_rng(31 + si)
    w = rng.uniform(0, 2, case["B"]).astype(np.float32) if extras else None
    off = rng.normal(0, 1, case["NI"]).astype(np.float32) if extras else None
    scale, l2_reg = 2.0, float(np.float32(0.01))
    tabs = _tables(rt, U, V, b)
    args = [None if x is None else (torch.from_numpy(x).cuda() if device else x) for x in (uid, pid, w, off)]
    loss, l2 = rt.fullsoftmax_step(rt.Optimizer.sgd(1.0), *tabs, args[0], args[1], weights=args[2], item_offset=args[3], scale=scale,
                                   l2_reg=l2_reg, chunk_items=case["chunk_items"], chunk_samples=case["chunk_samples"], precision="bf16")
    wl, wl2, g = ref_grads(U, V, b, uid, pid, w, off, scale, l2_reg)
    assert abs(loss[0] - wl) <= TOL * abs(wl) and abs(l2[0] - wl2) <= TOL * abs(wl2)
    gU, bU = np.zeros(U.shape), np.zeros(U.shape)
    np.add.at(gU, uid, g["gu"][0]); np.add.at(bU, uid, g["gu"][1])         # SGD accumulates every occurrence of a user
    for name, W0, t, (grad, bound) in (("user", U, tabs[0], (gU, bU)), ("item", V, tabs[1], g["GV"]), ("bias", b, tabs[2], g["Gb"])):
        if t is None:
            continue
        got, want = t.read(), (W0.astype(np.float64) - grad.reshape(W0.shape))
        if bound is None:                       # the bias gradient sums the unrounded coefficients: the fp32 path's check
            delta_check(W0, got, want.astype(np.float32), what=f"{case['name']} bias")
            continue
        ulp = np.spacing(np.maximum(np.maximum(np.abs(want), np.abs(W0)), np.abs(grad).max()).astype(np.float32)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - want)
        print(f"{case['name']} {name}: worst element {(err / (bound + 2 * ulp)).max():.3g} x bound")
        assert (err <= bound + 2 * ulp).all(), name
        assert not np.array_equal(got, W0)


# ---- 4. consistency ----------------------------------------------------------------------------------------------------------------
def test_forward_is_the_steps_loss_two_runs_agree_and_a_removed_item_keeps_its_bits():
    rt = _rt()
    case = fc.shape_case(4, seed=41)
    U, V, b, uid, pid = fc.make(case)
    off = np.random.default_rng(4).normal(0, 1, case["NI"]).astype(np.float32)
    gone = np.setdiff1d(np.arange(0, case["NI"], 97), pid)
    off[gone] = -np.inf
    kw = dict(item_offset=off, scale=2.0, chunk_items=case["chunk_items"], precision="bf16")
    runs = []
    for _ in range(2):
        tabs = _tables(rt, U, V, b)
        fwd = rt.fullsoftmax_loss(*tabs, uid, pid, **kw)
        loss, l2 = rt.fullsoftmax_step(rt.Optimizer.sgd(0.05), *tabs, uid, pid, chunk_samples=case["chunk_samples"], **kw)
        assert np.float32(fwd[0]).view(np.int32) == loss.view(np.int32)[0] and np.float32(fwd[1]).view(np.int32) == l2.view(np.int32)[0]
        runs.append([t.read().view(np.int32) for t in tabs] + [loss.view(np.int32), l2.view(np.int32)])
    assert all(np.array_equal(x, y) for x, y in zip(*runs))
    assert np.array_equal(runs[0][1][gone], V.view(np.int32)[gone]) and np.array_equal(runs[0][2][gone], b.view(np.int32)[gone])
    assert not np.array_equal(runs[0][1], V.view(np.int32))


@pytest.mark.parametrize("deep", [False, True])
def test_the_pooled_forms_score_their_query_rows_as_the_user_table_form_does(deep):
    rt = _rt()
    rng = np.random.default_rng(5)
    T = lambda rows, dim: rt.Table(rows, dim).write(rng.uniform(-0.3, 0.3, (rows, dim)).astype(np.float32))
    V, b, B = T(65, 8), T(65, 1), 33
    if deep:
        net = rt.DeepSeqRec(T(65, 6), V, b, [(T(9, 12), T(1, 12)), T(12, 8)], side=[T(7, 3)], relu_last=False)
        side = (rng.integers(0, 7, B).astype(np.int32),)
    else:
        net, side = rt.SeqRec(T(65, 8), V, b), ()
    ptr = np.concatenate([[0], np.cumsum(rng.integers(1, 5, B))]).astype(np.int32)
    bags, pid = (ptr, rng.integers(0, 65, ptr[-1]).astype(np.int32)), rng.integers(0, 65, B).astype(np.int32)
    Q = rt.Table(B, 8).write(net.user_table(bags, *((side,) if deep else ())).read())
    want = rt.fullsoftmax_loss(Q, V, b, np.arange(B, dtype=np.int32), pid, scale=2.0, per_row=True, precision="bf16")
    got = net.loss_full(bags, pid, *((side,) if deep else ()), scale=2.0, per_row=True, precision="bf16")
    loss, _ = net.step_full(rt.Optimizer.sgd(0.05), bags, pid, *((side,) if deep else ()), scale=2.0, precision="bf16")
    assert np.array_equal(got[2].view(np.int32), want[2].view(np.int32)) and got[0] == want[0] and np.float32(got[0]) == loss[0]
    assert not np.array_equal(got[2], net.loss_full(bags, pid, *((side,) if deep else ()), scale=2.0, per_row=True)[2])


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from openrec_amd import _ffi
    rt = _rt()
    rng = np.random.default_rng(6)
    T = lambda rows, dim: rt.Table(rows, dim).write(rng.uniform(-0.3, 0.3, (rows, dim)).astype(np.float32))
    U, H, V = T(10, 8), T(65, 8), T(65, 8)
    ids = np.arange(4, dtype=np.int32)
    with pytest.raises(ValueError, match="precision"):
        rt.fullsoftmax_loss(U, V, None, ids, ids, precision="fp8")
    net, sgd = rt.SeqRec(H, V, None), rt.Optimizer.sgd(0.05)
    ptr = np.arange(5, dtype=np.int32)
    with pytest.raises(ValueError, match="labels"):
        net.step_full(sgd, (ptr, ids), labels=(ptr, ids), precision="bf16")
    ctx = V.ctx
    with pytest.raises(ValueError, match="orx_seqrec_full_sets_step: ORX_FS_BF16"):
        _ffi.check(ctx._lib.orx_seqrec_full_sets_step(ctx._h, sgd._h, H._h, V._h, None, ptr.ctypes.data, ids.ctypes.data, ptr.ctypes.data,
                                                      ids.ctypes.data, None, 4, None, None, 4, 4, _ffi.ORX_BAG_MEAN, 1.0, 1.0, 0.0, 0, 0, 0,
                                                      _ffi.ORX_FS_BF16, None, None))
