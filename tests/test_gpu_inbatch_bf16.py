"""GPU: the in-batch softmax with bf16 operands on the matrix cores (precision="bf16", ORX_IB_BF16) against the rounded semantics of
include/openrec_hip.h in float64: inbatch_ref on float64(bf(U)), float64(bf(V)), bf(x) a torch.bfloat16 round trip.

Row losses are held to inbatch_ref.row_bound on the bf16-rounded tables: products of bf16 values are exact in fp32 and the
instruction sums them in fp32, so the fp32 path's bound holds as it stands.  A gradient element is held to
(2^-8 + TOL) * scale * sum |a| |bf(x)| + TOL |l2 term| + 2 ulp(W): 2^-9 is the coefficient's bf16 rounding, doubled for the device's
own a; TOL is fp32 accumulation; the ulp term is delta_check's.  The bias gradient sums unrounded coefficients: delta_check."""
import numpy as np
import pytest
import torch

import inbatch_cases as ic
import inbatch_ref as ir
from conftest import TOL, delta_check

pytestmark = pytest.mark.gpu


def _rt():
    from openrec_amd import runtime as rt
    return rt


def bf(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).bfloat16().float().numpy()


def _f64(x):
    return None if x is None else np.asarray(x, np.float64)


def _tables(rt, *arrays):
    return tuple(None if x is None else rt.Table(*x.shape).write(x) for x in arrays)


def _bits(tabs, *more):
    return [t.read().view(np.int32) for t in tabs if t is not None] + [np.asarray(x, np.float32).view(np.int32) for x in more]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _case(si, **kw):
    B, D, NU, NI, chunk = ic.SHAPES[si]
    return dict(dict(opt="sgd", bias=True, K=1, mask=True, B=B, D=D, NU=NU, NI=NI, chunk=chunk, seed=500 + si), **kw)


def _check_sgd_step(what, tabs, loss, l2, U, V, b, uid, pid, w, off, scale, mask, l2_reg):
    """tabs after ONE SGD step at lr = 1 from (U, V, b), and its losses (None: the call raised), against the rounded semantics in
    float64"""
    B, eye = len(uid), np.eye(len(uid), dtype=bool)
    u, v, s = ir.scores(_f64(bf(U)), _f64(bf(V)), _f64(b), uid, pid, _f64(off), scale)
    n = ir.columns(pid, mask)
    pi = np.where(n, np.exp(np.where(n, s, -np.inf) - ir._lse(s, n)[:, None]), 0.0)
    c = (np.ones(B) if w is None else _f64(w)) / B
    a = np.where(eye, -(c * np.where(eye, 0.0, pi).sum(1))[:, None], c[:, None] * pi)
    ab, k = _f64(bf(a)), 2.0 ** -8 + TOL
    wl = (c * (ir._lse(s, n) - np.diagonal(s))).sum()
    wl2 = 0.5 * ((_f64(U)[uid] ** 2).sum() + (_f64(V)[pid] ** 2).sum())
    assert loss is None or (abs(loss - wl) <= TOL * abs(wl) and abs(l2 - wl2) <= TOL * abs(wl2)), (what, loss, wl, l2, wl2)
    lu, lv = l2_reg * _f64(U)[uid], l2_reg * _f64(V)[pid]
    rows = ((U, uid, scale * ab @ v + lu, k * scale * np.abs(a) @ np.abs(v) + TOL * np.abs(lu)),
            (V, pid, scale * ab.T @ u + lv, k * scale * np.abs(a).T @ np.abs(u) + TOL * np.abs(lv)),
            (b, pid, (scale * a.sum(0))[:, None], None))
    for name, t, (W0, ids, g, gbound) in zip(("user", "item", "bias"), tabs, rows):
        if t is None:
            continue
        grad, bound = np.zeros(W0.shape), np.zeros(W0.shape)
        np.add.at(grad, ids, g)                                            # SGD accumulates every occurrence of a row
        got, want = t.read(), W0.astype(np.float64) - grad
        if gbound is None:
            delta_check(W0, got, want.astype(np.float32), what=f"{what} bias")
            continue
        np.add.at(bound, ids, gbound)
        ulp = np.spacing(np.maximum(np.maximum(np.abs(want), np.abs(W0)), np.abs(grad).max()).astype(np.float32)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - want)
        print(f"{what} {name}: worst element {(err / (bound + 2 * ulp)).max():.3g} x bound")
        assert (err <= bound + 2 * ulp).all(), (what, name)
        assert not np.array_equal(got, W0)


# ---- 1. row losses ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(1, len(ic.SHAPES)))
def test_every_row_loss_is_within_the_bound_of_the_rounded_tables(si):
    rt = _rt()
    case = _case(si)
    U, V, b, uid, pid = ic.make(case)
    off = np.random.default_rng(21 + si).normal(0, 1, case["B"]).astype(np.float32)
    tabs = _tables(rt, U, V, b)
    for scale in (1.0, 4.0):
        loss, l2, rows = rt.inbatch_loss(*tabs, uid[0], pid[0], item_offset=off, scale=scale, chunk=case["chunk"], per_row=True,
                                         precision="bf16")
        want = ir.row_losses(_f64(bf(U)), _f64(bf(V)), _f64(b), uid[0], pid[0], _f64(off), scale, True)
        bound = ir.row_bound(bf(U), bf(V), b, uid[0], pid[0], off, scale, True)
        err = np.abs(rows.astype(np.float64) - want)
        print(f"B={case['B']} D={case['D']} scale={scale}: worst row {(err / bound).max():.3g} x bound")
        assert rows.shape == (case["B"],) and (err <= bound).all(), float((err / bound).max())
        assert abs(loss - want.mean()) <= TOL * abs(want.mean())


# ---- 2. the rounding is where the semantics put it ----------------------------------------------------------------------------------
@pytest.mark.parametrize("si", [3, 4])
def test_the_rows_are_those_of_the_rounded_tables_and_not_of_the_fp32_tables(si):
    rt = _rt()
    case = _case(si)
    U, V, b, uid, pid = ic.make(case)
    rows = rt.inbatch_loss(*_tables(rt, U, V, b), uid[0], pid[0], chunk=case["chunk"], per_row=True, precision="bf16")[2].astype(np.float64)
    inside = np.abs(rows - ir.row_losses(_f64(bf(U)), _f64(bf(V)), _f64(b), uid[0], pid[0])) <= ir.row_bound(bf(U), bf(V), b, uid[0], pid[0])
    outside = np.abs(rows - ir.row_losses(_f64(U), _f64(V), _f64(b), uid[0], pid[0])) > ir.row_bound(U, V, b, uid[0], pid[0])
    print(f"B={case['B']} D={case['D']}: {outside.mean():.2f} of the rows outside the bound of the unrounded tables")
    assert inside.all() and outside.mean() > 0.5


# ---- 3. one SGD step with lr = 1: W0 - W1 is the gradient ---------------------------------------------------------------------------
@pytest.mark.parametrize("si,bias,extras,device,mask", [(3, True, False, False, True), (3, False, True, True, False), (4, True, True, False, True),
                                                        (5, False, False, True, False), (5, True, True, False, True), (6, True, True, True, False),
                                                        (2, False, False, False, True)])
def test_one_sgd_step_gives_the_gradients_of_the_rounded_semantics(si, bias, extras, device, mask):
    rt = _rt()
    case = _case(si, bias=bias, mask=mask, seed=900 + si)
    U, V, b, uid, pid = ic.make(case)
    rng = np.random.default_rng(31 + si)
    w = rng.uniform(0, 2, case["B"]).astype(np.float32) if extras else None
    off = rng.normal(0, 1, case["B"]).astype(np.float32) if extras else None
    scale, l2_reg = (2.0, float(np.float32(0.01))) if extras else (1.0, 1.0)
    tabs = _tables(rt, U, V, b)
    args = [None if x is None else (torch.from_numpy(x).cuda() if device else x) for x in (uid[0], pid[0], w, off)]
    loss, l2 = rt.inbatch_step(rt.Optimizer.sgd(1.0), *tabs, args[0], args[1], weights=args[2], item_offset=args[3], scale=scale,
                               mask_hits=mask, l2_reg=l2_reg, chunk=case["chunk"], precision="bf16")
    _check_sgd_step(f"B={case['B']} D={case['D']}", tabs, loss[0], l2[0], U, V, b, uid[0], pid[0], w, off, scale, mask, l2_reg)


# ---- 4. consistency ----------------------------------------------------------------------------------------------------------------
def test_forward_is_the_steps_loss_and_two_runs_agree():
    rt = _rt()
    case = _case(4, bias=False, seed=41)
    U, V, b, uid, pid = ic.make(case)
    off = np.random.default_rng(4).normal(0, 1, case["B"]).astype(np.float32)
    kw = dict(item_offset=off, scale=2.0, chunk=case["chunk"], precision="bf16")
    runs = []
    for _ in range(2):
        tabs = _tables(rt, U, V, b)
        fwd = rt.inbatch_loss(*tabs, uid[0], pid[0], **kw)
        loss, l2 = rt.inbatch_step(rt.Optimizer.sgd(0.05), *tabs, uid[0], pid[0], **kw)
        assert _same(_bits((), fwd[0], fwd[1]), _bits((), loss[0], l2[0]))
        runs.append(_bits(tabs, loss, l2))
    assert _same(*runs) and not np.array_equal(runs[0][0], U.view(np.int32))
    assert loss[0] != rt.inbatch_loss(*_tables(rt, U, V, b), uid[0], pid[0], item_offset=off, scale=2.0, chunk=case["chunk"])[0]


def test_three_adam_steps_in_one_call_are_three_calls():
    rt = _rt()
    case = _case(4, bias=False, K=3, seed=42)
    U, V, b, uid, pid = ic.make(case)
    one, three = _tables(rt, U, V, b), _tables(rt, U, V, b)
    l_one = rt.inbatch_step(rt.Optimizer.adam(0.002), *one, uid, pid, K=3, chunk=64, precision="bf16")
    o = rt.Optimizer.adam(0.002)
    l_three = [rt.inbatch_step(o, *three, uid[s], pid[s], chunk=64, precision="bf16") for s in range(3)]
    assert _same(_bits(one, *l_one), _bits(three, *(np.concatenate([x[i] for x in l_three]) for i in range(2))))


def test_host_and_device_ids_give_the_same_bits():
    rt = _rt()
    case = _case(3, bias=False, K=2, seed=43)
    U, V, b, uid, pid = ic.make(case)
    host, dev = _tables(rt, U, V, b), _tables(rt, U, V, b)
    lh = rt.inbatch_step(rt.Optimizer.sgd(0.05), *host, uid, pid, K=2, precision="bf16")
    ld = rt.inbatch_step(rt.Optimizer.sgd(0.05), *dev, torch.from_numpy(uid).cuda(), torch.from_numpy(pid).cuda(), K=2, precision="bf16")
    assert _same(_bits(host, *lh), _bits(dev, *ld))


@pytest.mark.parametrize("which", ["uid", "pid"])
def test_an_id_out_of_range_raises_and_leaves_the_good_samples_alone(which):
    """the tables after the refused call are those of the batch without the bad sample (weights (B - 1) / B keep c_i = 1 / B)"""
    rt = _rt()
    case = _case(4, NU=200, NI=300, seed=44)
    U, V, b, uid, pid = ic.make(case)
    tabs = _tables(rt, U, V, b)
    u, p, k = uid[0].copy(), pid[0].copy(), 71
    if which == "uid":
        u[k] = case["NU"] + 3
    else:
        p[k] = -1
    with pytest.raises(IndexError):
        rt.inbatch_step(rt.Optimizer.sgd(1.0), *tabs, u, p, chunk=64, precision="bf16")
    keep = np.arange(case["B"]) != k
    _check_sgd_step(f"{which} out of range", tabs, None, None, U, V, b, uid[0][keep], pid[0][keep], np.full(129, 129.0 / 130.0), None, 1.0, True, 1.0)


def test_bpr_train_steps_inbatch_is_the_runtime_call_and_an_unknown_precision_is_refused():
    rt = _rt()
    from openrec_amd.tf2.recommenders import BPR
    case = _case(3, bias=False, K=2, seed=45)
    U, V, _, uid, pid = ic.make(case)
    model = BPR(64, 64, case["NU"], case["NI"], use_item_bias=False, l2_reg=0.01)
    model.user_latent_factor.table.write(U); model.item_latent_factor.table.write(V)
    got = model.train_steps_inbatch(rt.Optimizer.adagrad(0.05), uid, pid, scale=2.0, precision="bf16")
    tabs = _tables(rt, U, V, None)
    want = rt.inbatch_step(rt.Optimizer.adagrad(0.05), *tabs, uid, pid, K=2, scale=2.0, l2_reg=0.01, precision="bf16")
    assert _same(_bits((model.user_latent_factor.table, model.item_latent_factor.table), *got), _bits(tabs, *want))
    fp32 = _tables(rt, U, V, None)
    rt.inbatch_step(rt.Optimizer.adagrad(0.05), *fp32, uid, pid, K=2, scale=2.0, l2_reg=0.01)
    assert not _same(_bits(tabs), _bits(fp32))
    for call in (lambda: rt.inbatch_step(rt.Optimizer.sgd(0.05), *tabs, uid, pid, K=2, precision="fp8"),
                 lambda: rt.inbatch_loss(*tabs, uid[0], pid[0], precision="fp8")):
        with pytest.raises(ValueError, match="precision"):
            call()
