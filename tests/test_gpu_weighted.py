"""GPU: train steps with per-triplet weights and an l2 coefficient (`rt.pairwise_step(weights=, l2_reg=)`,
`rt.pairwise_loss(weights=)`, `rt.pointwise_step(l2_reg=)`, `DeviceSampler.pairwise_weights`, the tf2 recommenders' `l2_reg` and
`sample_weight`) against tests/weighted_ref.py, the expectation composed from the unchanged oracle (held to the reference's own
class text by tests/test_weighted_cpu.py).  Tolerances are the project's: conftest.delta_check on tables, TOL on slots, loss and
l2, TOL_ADAM for Adam.  Where two routes can be compared bit for bit (inputs on which every row has at most two references) they
are: the weighted entry point with all-ones weights and coefficient 1 IS the plain step.

The expectation is computed in float64 and rounded to float32 once.  With a small coefficient the l2 part of an update no longer
dominates it, and delta_check's bound is then its ulp term alone: (steps + 1) ulp of the table's values, one rounding per step
and implementation.  A float32 NumPy oracle does not round once per step on these inputs: its SGD subtracts lr * g occurrence
by occurrence, and a row referenced r times in a step (r reaches 10 with 1024 item references over 400 rows) collects r
roundings at the ulp of the table's values where the device sums the r small gradients first and rounds the row once.  That
error is the reference's own, so it is taken out of the reference rather than added to the bound.

Adam's learning rate is chosen per model so that TOL_ADAM applies.  conftest derives TOL_ADAM for lr = 2e-3 and a summed gradient
whose terms are 0.05-sized: where an element's summed gradient nearly cancels, its fp32 rounding delta enters the update as
lr * sqrt(1 - beta_2) * delta / eps, i.e. lr * delta * 6.3e6 of the tables' 0.05 range -- 3.8e-5 at delta = 3e-9.  BPR fits that:
its loss gradient carries 1/B and the l2 term is a table value.  UCML does not: the hinge gradient of one reference is
2 w (p - n), up to 0.4 at w < 2, it is not divided by B, and on these inputs an item row sums about ten of them, so partial sums
reach 1 and delta is half an ulp of that, 6e-8.  The same formula then asks for lr <= 3.8e-5 / (6e-8 * 6.3e6) = 1e-4.  At
lr = 2e-3 the plain, unweighted step misses TOL_ADAM on this shape as well (UCML, D = 128, the inputs of seed 2: user table
5.1e-5; with weights, seed 0: item table 6.1e-5 to 1.0e-4 from run to run), so the figure says nothing about the weights.  The
optimizer slots, whose error does not scale with lr, are held to TOL_ADAM at either rate and are what resolves a wrong weight."""
import os

import numpy as np
import pytest

import weighted_ref as wr
from conftest import TOL, TOL_ADAM, delta_check, rel_err
from subset_expect import Momentum

pytestmark = pytest.mark.gpu

NU, NI, B, K, STRIDE = 300, 400, 512, 3, 640
OPTS = ("sgd", "adagrad", "adam", "momentum")
LR = {"sgd": 0.05, "adagrad": 0.05, "adam": 0.002, "momentum": 0.05}
LR_ADAM = {"bpr": 2e-3, "ucml": 1e-4}         # (see the module docstring)
KEY = {"user": "U", "item": "V", "bias": "b"}


def _rt():
    from openrec_amd import runtime as rt
    return rt


def _opts(name, rt, ctx=None, beta_1=0.9, model="bpr"):
    """(device optimizer, oracle optimizer)"""
    from oracle import numpy_oracle as orc
    lr = LR_ADAM[model] if name == "adam" else LR[name]
    if name == "sgd":
        return rt.Optimizer.sgd(lr, ctx=ctx), orc.SGD(lr)
    if name == "adagrad":
        return rt.Optimizer.adagrad(lr, ctx=ctx), orc.Adagrad(lr)
    if name == "adam":
        return rt.Optimizer.adam(lr, beta_1=beta_1, ctx=ctx), orc.AdamTFSparse(lr, beta_1=beta_1)
    return rt.Optimizer.momentum(lr, 0.9, True, ctx=ctx), Momentum(lr, 0.9, True)


def _oslots(oo, key):
    if oo.kind == "adagrad":
        return [oo.acc[key]]
    if oo.kind == "adam":
        return [oo.m[key], oo.v[key]]
    if oo.kind == "momentum":
        return [oo.vel[key]]
    return []


def _weights(rng, shape):
    """uniform in [0, 2) with about 10 % exact zeros"""
    w = rng.uniform(0, 2, shape).astype(np.float32)
    w[rng.random(shape) < 0.1] = 0.0
    return w


def _case(seed, D, nu=NU, ni=NI, scale=0.05):
    """ids and weights laid out at STRIDE > B: the gap holds ids out of range and NaN weights, which a wrong stride would read"""
    rng = np.random.default_rng(seed)
    U = rng.uniform(-scale, scale, (nu, D)).astype(np.float32); V = rng.uniform(-scale, scale, (ni, D)).astype(np.float32)
    b = rng.uniform(-scale, scale, (ni, 1)).astype(np.float32)
    ids = np.full((3, K, STRIDE), -7, np.int32)
    ids[0, :, :B] = rng.integers(0, nu, (K, B)); ids[1, :, :B] = rng.integers(0, ni, (K, B)); ids[2, :, :B] = rng.integers(0, ni, (K, B))
    w = np.full((K, STRIDE), np.nan, np.float32)
    w[:, :B] = _weights(rng, (K, B))
    assert (w[:, :B] == 0).sum() > K * B // 20
    return U, V, b, ids[0], ids[1], ids[2], w


def _dev(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in arrays)


def _f64(*arrays):
    return tuple(x.astype(np.float64) for x in arrays)


def _check_tables(what, optname, tabs, host, orig, opt, oo, roles, steps):
    """host: the float64 expectation, rounded to float32 here; orig: the float32 tables before the call"""
    host = {r: (x.astype(np.float32) if x is not None else None) for r, x in host.items()}
    for r in roles:
        got = tabs[r].read()
        print(f"{what} {r}: rel err {rel_err(got, host[r]):.3g}")
        if optname == "adam":
            d_got, d_want = got.astype(np.float64) - orig[r], host[r].astype(np.float64) - orig[r]
            print(f"{what} {r}: update projected on the expected update {float((d_got * d_want).sum() / (d_want * d_want).sum()):.6f}")
            assert rel_err(got, host[r]) <= TOL_ADAM, (what, r)
        else:
            delta_check(orig[r], got, host[r], steps=steps, what=f"{what} {r}")
        for k, want in enumerate(_oslots(oo, KEY[r])):
            e = rel_err(opt.slot(tabs[r], k), want)
            print(f"{what} {r} slot {k}: rel err {e:.3g}")
            assert e <= (TOL_ADAM if optname == "adam" else TOL), (what, r, k, e)


def _check_losses(what, loss, l2, want):
    for s, (lw, l2w) in enumerate(want):
        print(f"{what} step {s}: loss {loss[s]:.8g} want {lw:.8g}  l2 {l2[s]:.8g} want {l2w:.8g}")
        assert abs(loss[s] - lw) <= TOL * abs(lw) and abs(l2[s] - l2w) <= TOL * abs(l2w), (what, s, loss[s], lw, l2[s], l2w)


def _run_pair(model, optname, D, l2_reg, has_bias=True, device=False, censor=False, roles=wr.ALL, seed=0, nu=NU, ni=NI, beta_1=0.9,
              scale=0.05):
    rt = _rt()
    U, V, b, uid, pid, nid, w = _case(seed + D, D, nu, ni, scale)
    tU = rt.Table(nu, D).write(U); tV = rt.Table(ni, D).write(V); tb = rt.Table(ni, 1).write(b) if has_bias else None
    tabs = {"user": tU, "item": tV, "bias": tb}
    orig = {r: x.copy() for r, x in (("user", U), ("item", V), ("bias", b)) if tabs[r] is not None}
    U, V, b = _f64(U, V, b)
    hb = b if has_bias else None
    opt, oo = _opts(optname, rt, beta_1=beta_1, model=model)
    live = tuple(r for r in roles if tabs[r] is not None)
    frozen = [r for r in wr.ALL if r not in live and tabs[r] is not None]
    before = {r: tabs[r].read() for r in frozen}
    args = (uid.reshape(-1), pid.reshape(-1), nid.reshape(-1))
    wa = w.reshape(-1)
    if device:
        args = _dev(*args); wa, = _dev(wa)
    loss, l2 = rt.pairwise_step(model, opt, tU, tV, tb, *args, K=K, B=B, id_stride=STRIDE, margin=0.5, weights=wa, l2_reg=l2_reg,
                                censor=censor, train=None if len(live) == len([t for t in tabs.values() if t is not None]) else live)
    want = [wr.pair_step(model, U, V, hb, uid[s, :B], pid[s, :B], nid[s, :B], oo, w=w[s, :B], l2_reg=l2_reg, roles=live, censor=censor)
            for s in range(K)]
    what = f"{model}{'' if has_bias else '_nb'} {optname} D={D} l2_reg={l2_reg} {'device' if device else 'host'} ids"
    _check_losses(what, loss, l2, want)
    for r in frozen:
        assert np.array_equal(before[r], tabs[r].read()), f"{what}: frozen {r} moved"
    _check_tables(what, optname, tabs, {"user": U, "item": V, "bias": hb}, orig, opt, oo, live, K)
    return tabs, opt


@pytest.mark.parametrize("D", [50, 64, 128])
@pytest.mark.parametrize("optname", OPTS)
@pytest.mark.parametrize("model", ["bpr", "ucml", "bpr_nb"])
def test_small_duplicate_heavy_step_matches_the_weighted_reference(model, optname, D):
    """512 triplets over 300 users and 400 items: rows referenced twice, three times and more; weights with exact zeros; the ids'
    stride on the weights; every coefficient with host ids, and 0.01 with device ids and weights too"""
    m, hb = ("bpr", False) if model == "bpr_nb" else (model, True)
    for l2_reg in (0.0, 0.01, 1.0):
        _run_pair(m, optname, D, l2_reg, has_bias=hb)
    _run_pair(m, optname, D, 0.01, has_bias=hb, device=True, seed=1)


def test_ucml_with_the_censor_folded_in():
    _run_pair("ucml", "sgd", 64, 0.01, censor=True)


@pytest.mark.parametrize("nu,beta_1", [(NU, 0.97), (40000, 0.97), (40000, 0.9)])
def test_lazy_adam_replays(nu, beta_1):
    """the three replays of lazy Adam with weights: the merged loop (beta_1 outside the closed form's range), the bounded per-row
    replay beside it (tables large against the batch), and the closed form"""
    _run_pair("bpr", "adam", 64, 0.01, nu=nu, ni=nu, beta_1=beta_1, device=True)


@pytest.mark.parametrize("roles", [("user",), ("item", "bias")])
@pytest.mark.parametrize("optname", ["sgd", "adam"])
@pytest.mark.parametrize("D", [50, 64])
def test_strict_subsets_take_the_weights_and_the_coefficient(roles, optname, D):
    """frozen tables bit for bit against their values before the call (checked in _run_pair)"""
    _run_pair("bpr", optname, D, 0.01, roles=roles)


# ---- inputs on which two routes can be compared bit for bit ---------------------------------------------------------------------
def _twice():
    from test_gpu_subset import _twice_case
    return _twice_case(9, 64)


def _fresh(rt, U, V, b, optname, ctx=None):
    tU, tV, tb = (rt.Table(*x.shape, ctx).write(x) for x in (U, V, b))
    return tU, tV, tb, _opts(optname, rt, ctx)[0]


def _state(tU, tV, tb, opt, nslot):
    return [t.read() for t in (tU, tV, tb)] + [opt.slot(t, k) for t in (tU, tV, tb) for k in range(nslot)]


def _same(a, b):
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("optname,nslot", [("sgd", 0), ("adagrad", 1), ("adam", 2)])
def test_unit_weights_and_coefficient_one_are_the_plain_step_bit_for_bit(optname, nslot):
    rt = _rt()
    U, V, b, uid, pid, nid, _ = _twice()
    Kt, Bt = uid.shape
    ids = (uid.reshape(-1), pid.reshape(-1), nid.reshape(-1))
    res = []
    for kw in ({}, dict(weights=np.ones(Kt * Bt, np.float32), l2_reg=1.0), dict(no_l2=True), dict(l2_reg=0.0)):
        tU, tV, tb, opt = _fresh(rt, U, V, b, optname)
        loss, l2 = rt.pairwise_step("bpr", opt, tU, tV, tb, *ids, K=Kt, B=Bt, **kw)
        res.append(_state(tU, tV, tb, opt, nslot) + [loss, l2])
    assert _same(res[0], res[1]), "weights = 1, l2_reg = 1 differs from the plain step"
    assert _same(res[2], res[3]), "l2_reg = 0 differs from no_l2"
    assert not _same(res[0][:3], res[2][:3])


def test_pairing_reads_the_weight_at_the_triplets_original_position():
    """every user referenced exactly twice: the plan pairs triplets and moves them; weights distinct per triplet"""
    from test_gpu_pairing import env
    rt = _rt()
    U, V, b, uid, pid, nid, _ = _twice()
    Kt, Bt = uid.shape
    w = (1.0 + np.arange(Kt * Bt, dtype=np.float32).reshape(Kt, Bt) % Bt / Bt).astype(np.float32)
    with env(ORX_PAIR_ALWAYS=1, ORX_NO_PAIR=None):
        ctx = rt.Context(0)
        tU, tV, tb, opt = _fresh(rt, U, V, b, "sgd", ctx)
        loss, l2 = rt.pairwise_step("bpr", opt, tU, tV, tb, uid.reshape(-1), pid.reshape(-1), nid.reshape(-1), K=Kt, B=Bt,
                                    weights=w.reshape(-1), l2_reg=0.01)
        pairs = ctx.stat("pairs")
    assert pairs > 0, "pairing was idle"
    from oracle import numpy_oracle as orc
    oo = orc.SGD(LR["sgd"])
    orig = dict(user=U.copy(), item=V.copy(), bias=b.copy())
    U, V, b = _f64(U, V, b)
    want = [wr.pair_step("bpr", U, V, b, uid[s], pid[s], nid[s], oo, w=w[s], l2_reg=0.01) for s in range(Kt)]
    _check_losses("pairing", loss, l2, want)
    _check_tables(f"pairing ({pairs} pairs)", "sgd", dict(user=tU, item=tV, bias=tb), dict(user=U, item=V, bias=b), orig, opt, oo, wr.ALL, Kt)


@pytest.mark.parametrize("optname,nslot", [("sgd", 0), ("adam", 2)])
def test_one_call_of_k_steps_equals_k_calls(optname, nslot):
    rt = _rt()
    U, V, b, uid, pid, nid, _ = _twice()
    Kt, Bt = uid.shape
    w = _weights(np.random.default_rng(3), (Kt, Bt))
    tU, tV, tb, opt = _fresh(rt, U, V, b, optname)
    loss, l2 = rt.pairwise_step("bpr", opt, tU, tV, tb, uid.reshape(-1), pid.reshape(-1), nid.reshape(-1), K=Kt, B=Bt, weights=w.reshape(-1), l2_reg=0.01)
    one = _state(tU, tV, tb, opt, nslot) + [loss, l2]
    tU, tV, tb, opt = _fresh(rt, U, V, b, optname)
    outs = [rt.pairwise_step("bpr", opt, tU, tV, tb, uid[s], pid[s], nid[s], K=1, B=Bt, weights=w[s], l2_reg=0.01) for s in range(Kt)]
    many = _state(tU, tV, tb, opt, nslot) + [np.array([o[0][0] for o in outs]), np.array([o[1][0] for o in outs])]
    assert _same(one, many)


@pytest.mark.parametrize("model,optname,D", [("bpr", "sgd", 64), ("bpr", "adagrad", 64), ("bpr", "adam", 64), ("ucml", "sgd", 50),
                                             ("ucml", "momentum", 128)])
def test_one_call_of_k_steps_equals_k_calls_on_the_duplicate_heavy_case(model, optname, D):
    """rows referenced three times and more: staging, atomics and the in-launch apply across step boundaries in the K-step call,
    separate applies in the one-step calls.  Such rows sum in an order the plan chooses, so the two agree at tolerance: the tables
    of the one-step calls stand where the expectation stands in the other tests"""
    rt = _rt()
    U, V, b, uid, pid, nid, w = _case(50 + D, D)
    res = []
    for split in (False, True):
        tU = rt.Table(NU, D).write(U); tV = rt.Table(NI, D).write(V); tb = rt.Table(NI, 1).write(b)
        opt, _ = _opts(optname, rt, model=model)
        kw = dict(B=B, margin=0.5, l2_reg=0.01)
        if split:
            outs = [rt.pairwise_step(model, opt, tU, tV, tb, uid[s, :B], pid[s, :B], nid[s, :B], K=1, weights=w[s, :B], **kw) for s in range(K)]
            loss, l2 = np.array([o[0][0] for o in outs]), np.array([o[1][0] for o in outs])
        else:
            loss, l2 = rt.pairwise_step(model, opt, tU, tV, tb, uid.reshape(-1), pid.reshape(-1), nid.reshape(-1), K=K, id_stride=STRIDE,
                                        weights=w.reshape(-1), **kw)
        nslot = {"sgd": 0, "adagrad": 1, "adam": 2, "momentum": 1}[optname]
        res.append(([tU.read(), tV.read(), tb.read()], [opt.slot(t, k) for t in (tU, tV, tb) for k in range(nslot)], loss, l2))
    (t1, s1, loss1, l21), (tk, sk, lossk, l2k) = res
    what = f"K-step against one-step calls, {model} {optname} D={D}"
    _check_losses(what, loss1, l21, list(zip(lossk, l2k)))
    for name, W0, got, want in zip(("user", "item", "bias"), (U, V, b), t1, tk):
        print(f"{what} {name}: rel err {rel_err(got, want):.3g}")
        if optname == "adam":
            assert rel_err(got, want) <= TOL_ADAM, (what, name)
        else:
            delta_check(W0, got, want, steps=K, what=f"{what} {name}")
    for k, (x, y) in enumerate(zip(s1, sk)):
        assert rel_err(x, y) <= (TOL_ADAM if optname == "adam" else TOL), (what, "slot", k)


@pytest.mark.parametrize("D", [50, 64])
@pytest.mark.parametrize("model", ["bpr", "ucml", "bpr_nb"])
def test_weighted_forward(model, D):
    rt = _rt()
    U, V, b, uid, pid, nid, w = _case(21 + D, D)
    nb = model == "bpr_nb"
    m = "bpr" if nb else model
    tU = rt.Table(NU, D).write(U); tV = rt.Table(NI, D).write(V); tb = None if nb else rt.Table(NI, 1).write(b)
    hb = np.zeros_like(b) if nb else b
    want = wr.pair_forward(m, *_f64(U, V, hb), uid[0, :B], pid[0, :B], nid[0, :B], w[0, :B])
    for dev in (False, True):
        args = (uid[0, :B], pid[0, :B], nid[0, :B], w[0, :B])
        if dev:
            args = _dev(*args)
        got = rt.pairwise_loss(m, tU, tV, tb, *args[:3], margin=0.5, weights=args[3])
        _check_losses(f"forward {model} D={D}", [got[0]], [got[1]], [want])
    plain = rt.pairwise_loss(m, tU, tV, tb, uid[0, :B], pid[0, :B], nid[0, :B], margin=0.5)
    assert abs(plain[0] - want[0]) > 1e-3 * abs(want[0])            # (the weights are not ignored)


@pytest.mark.parametrize("D", [50, 64])
@pytest.mark.parametrize("optname", ["sgd", "adam"])
@pytest.mark.parametrize("model", ["wrmf", "wrmf_sigmoid", "gmf"])
def test_pointwise_step_with_an_l2_coefficient(model, optname, D):
    rt = _rt()
    rng = np.random.default_rng(31 + D)
    U, V, b, uid, pid, _, _ = _case(31 + D, D)
    uid, iid = np.ascontiguousarray(uid[:, :B]), np.ascontiguousarray(pid[:, :B])
    lab = (rng.random((K, B)) < 0.3).astype(np.float32)
    wd = rng.uniform(-.3, .3, (D, 1)).astype(np.float32)
    gmf, sig = model == "gmf", model == "wrmf_sigmoid"
    tU = rt.Table(NU, D).write(U); tV = rt.Table(NI, D).write(V); tb = rt.Table(NI, 1).write(b); tw = rt.Table(D, 1).write(wd) if gmf else None
    opt, oo = _opts(optname, rt)
    orig = dict(user=U.copy(), item=V.copy(), bias=b.copy(), w=wd.copy())
    U, V, b, wd, lab64 = _f64(U, V, b, wd, lab)
    kw = {} if gmf else dict(a=2.0, b_w=0.5, sigmoid=sig)
    loss, l2 = rt.pointwise_step("gmf" if gmf else "wrmf", opt, tU, tV, tb, tw, uid.reshape(-1), iid.reshape(-1), lab.reshape(-1), K=K, B=B,
                                 l2_reg=0.01, **kw)
    want = [wr.point_step("gmf" if gmf else "wrmf", U, V, b, wd if gmf else None, uid[s], iid[s], lab64[s], oo, l2_reg=0.01, **kw) for s in range(K)]
    what = f"{model} {optname} D={D} l2_reg=0.01"
    _check_losses(what, loss, l2, want)
    _check_tables(what, optname, dict(user=tU, item=tV, bias=tb), dict(user=U, item=V, bias=b), orig, opt, oo, wr.ALL, K)
    if gmf:
        got, wd = tw.read(), wd.astype(np.float32)
        print(f"{what} w: rel err {rel_err(got, wd):.3g}")
        if optname == "adam":
            assert rel_err(got, wd) <= TOL_ADAM
        else:
            delta_check(orig["w"], got, wd, steps=K, what=what + " w")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,word", [(dict(hogwild=True, l2_reg=0.01), "HOGWILD"), (dict(l2_reg=-0.5), "l2_reg"), (dict(l2_reg=float("nan")), "l2_reg"),
                                      (dict(l2_reg=float("inf")), "l2_reg"), (dict(l2_reg=0.01, train=("user",), censor=True), "CENSOR"),
                                      (dict(l2_reg=0.01, bias=None, model="ucml"), "bias")])
def test_refusals_name_the_cause_and_touch_nothing(kw, word):
    rt = _rt()
    U, V, b, uid, pid, nid, w = _case(41, 64)
    tU = rt.Table(NU, 64).write(U); tV = rt.Table(NI, 64).write(V); tb = rt.Table(NI, 1).write(b)
    opt = rt.Optimizer.sgd(0.05)
    kw = dict(kw)
    model = kw.pop("model", "bpr")
    bias = kw.pop("bias", tb)
    with pytest.raises(ValueError, match=word):
        rt.pairwise_step(model, opt, tU, tV, bias, uid[0, :B], pid[0, :B], nid[0, :B], weights=w[0, :B], **kw)
    assert np.array_equal(tU.read(), U) and np.array_equal(tV.read(), V) and np.array_equal(tb.read(), b)


def test_no_l2_flag_with_a_coefficient_is_refused_by_the_library():
    """the runtime raises on no_l2 with l2_reg before it calls; the C entry points refuse the flag themselves"""
    from openrec_amd import _ffi
    rt = _rt()
    U, V, b, uid, pid, nid, w = _case(43, 64)
    tU = rt.Table(NU, 64).write(U); tV = rt.Table(NI, 64).write(V); tb = rt.Table(NI, 1).write(b)
    opt = rt.Optimizer.sgd(0.05)
    u, p, n, ww = (np.ascontiguousarray(x[0, :B]) for x in (uid, pid, nid, w))
    lib = tU.ctx._lib
    rc = lib.orx_pairwise_step_weighted(tU.ctx._h, _ffi.ORX_BPR, opt._h, tU._h, tV._h, tb._h, u.ctypes.data, p.ctypes.data, n.ctypes.data,
                                        ww.ctypes.data, 1, B, B, 0.5, 0.01, _ffi.ORX_NO_L2, 0, None, None)
    assert rc == _ffi.ORX_ERR_ARG and b"ORX_NO_L2" in lib.orx_last_error()
    lab = np.zeros(B, np.float32)
    rc = lib.orx_pointwise_step_l2reg(tU.ctx._h, _ffi.ORX_WRMF, opt._h, tU._h, tV._h, tb._h, None, u.ctypes.data, p.ctypes.data, lab.ctypes.data,
                                      1, B, B, 1.0, 1.0, 0.01, _ffi.ORX_NO_L2, 0, None, None)
    assert rc == _ffi.ORX_ERR_ARG and b"ORX_NO_L2" in lib.orx_last_error()
    rc = lib.orx_pointwise_step_l2reg(tU.ctx._h, _ffi.ORX_WRMF, opt._h, tU._h, tV._h, tb._h, None, u.ctypes.data, p.ctypes.data, lab.ctypes.data,
                                      1, B, B, 1.0, 1.0, -1.0, 0, 0, None, None)
    assert rc == _ffi.ORX_ERR_ARG and b"l2_reg" in lib.orx_last_error()
    assert np.array_equal(tU.read(), U) and np.array_equal(tV.read(), V) and np.array_equal(tb.read(), b)
    with pytest.raises(ValueError, match="HOGWILD"):
        rt.pointwise_step("wrmf", opt, tU, tV, tb, None, u, p, lab, hogwild=True, l2_reg=0.01)
    with pytest.raises(ValueError, match="on the host with ids on the device"):
        rt.pairwise_step("bpr", opt, tU, tV, tb, *_dev(u, p, n), weights=ww)


# ---- the sampler's record weights -------------------------------------------------------------------------------------------------
SNU, SNI, NREC = 200, 150, 1000


@pytest.fixture(scope="module")
def records():
    """unique (user, item) records with distinct weights"""
    rng = np.random.default_rng(2)
    key = rng.permutation(SNU * SNI)[:NREC]
    raw = np.zeros(NREC, dtype=[("user_id", np.int32), ("item_id", np.int32)])
    raw["user_id"] = key // SNI; raw["item_id"] = key % SNI
    w = (0.25 + rng.permutation(NREC) / NREC).astype(np.float32)
    assert np.unique(w).size == NREC
    return raw, w, {int(k): float(x) for k, x in zip(key, w)}


@pytest.mark.parametrize("proposal", [False, True])
@pytest.mark.parametrize("hard", [False, True])
@pytest.mark.parametrize("first,n", [(0, 257), (900, 300), (123, 1)])
def test_sampler_delivers_the_weight_of_each_positive(records, proposal, hard, first, n):
    """w_dev[i] is the host weight of the record (uid[i], pid[i]) bit for bit -- from 0, from the middle, and across the epoch
    boundary at sample 1000; with and without a proposal; for the plain and the hard-negative draw"""
    import torch
    rt = _rt()
    raw, w, by_key = records
    sm = rt.Sampler(raw, SNU, SNI)
    if proposal:
        sm.set_proposal(popularity=0.75)
    sm.set_record_weights(w)
    dev = torch.device("cuda", 0)
    u, p, ng = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    wd = torch.full((n + 3,), -1.0, dtype=torch.float32, device=dev)
    if hard:
        tU = rt.Table(SNU, 16).init_uniform(-.5, .5, seed=1); tV = rt.Table(SNI, 16).init_uniform(-.5, .5, seed=2)
        sm.pairwise_hard(11, first, n, u, p, ng, "bpr", tU, tV, None, candidates=4)
    else:
        sm.pairwise(11, first, n, u, p, ng)
    sm.pairwise_weights(11, first, n, wd)
    sm.ctx.synchronize()
    got = wd.cpu().numpy()
    want = np.array([by_key[int(a) * SNI + int(c)] for a, c in zip(u.cpu().numpy(), p.cpu().numpy())], np.float32)
    assert np.array_equal(got[:n].view(np.int32), want.view(np.int32))
    assert (got[n:] == -1.0).all()                                # nothing written past n
    if first == 900:
        assert np.unique(got[:100]).size == 100                   # the tail of epoch 0: every record once


def test_sampler_without_record_weights_is_a_state_error(records):
    import torch
    from openrec_amd import _ffi
    rt = _rt()
    raw, w, _ = records
    sm = rt.Sampler(raw, SNU, SNI)
    out = torch.zeros(8, dtype=torch.float32, device=torch.device("cuda", 0))
    with pytest.raises(_ffi.OrxError) as e:
        sm.pairwise_weights(1, 0, 8, out)
    assert e.value.code == _ffi.ORX_ERR_STATE and "record weights" in str(e.value)
    sm.set_record_weights(w)
    sm.pairwise_weights(1, 0, 0, out)                             # n = 0: fine, nothing launched
    sm.pairwise_weights(1, 0, 8, out)
    sm.set_record_weights(None)
    with pytest.raises(_ffi.OrxError):
        sm.pairwise_weights(1, 0, 8, out)
    with pytest.raises(ValueError, match="999 weights for 1000 records"):
        sm.set_record_weights(w[:-1])


# ---- the tf2 recommenders ---------------------------------------------------------------------------------------------------------
def test_bpr_with_l2_reg_and_sample_weight_through_the_step_queue():
    """33 steps with sample_weight alternating with unweighted ones: the queue key keeps them apart and carries the weights; the
    second output of the call is l2_reg * l2_loss"""
    from openrec_amd.tf2 import compat as tf
    from openrec_amd.tf2 import recommenders as R
    from oracle import numpy_oracle as orc
    rng = np.random.default_rng(5)
    nu, ni, D, Bq = 700, 900, 64, 512
    m = R.BPR(dim_user_embed=D, dim_item_embed=D, total_users=nu, total_items=ni, l2_reg=0.01)
    U = rng.uniform(-.05, .05, (nu, D)).astype(np.float32); V = rng.uniform(-.05, .05, (ni, D)).astype(np.float32)
    b = rng.uniform(-.05, .05, (ni, 1)).astype(np.float32)
    orig = dict(user=U.copy(), item=V.copy(), bias=b.copy())
    m.user_latent_factor.variables[0].assign(U); m.item_latent_factor.variables[0].assign(V); m.item_bias.variables[0].assign(b)
    U, V, b = _f64(U, V, b)
    optimizer = tf.keras.optimizers.SGD(0.02)
    oo = orc.SGD(0.02)
    got, want = [], []
    n_w = 0
    for s in range(66):
        u = rng.integers(0, nu, Bq).astype(np.int32); p = rng.integers(0, ni, Bq).astype(np.int32); n = rng.integers(0, ni, Bq).astype(np.int32)
        # runs of weighted steps (long enough to queue several) between unweighted ones
        weighted = (s // 3) % 2 == 0
        w = _weights(rng, Bq) if weighted else None
        n_w += weighted
        with tf.GradientTape() as tape:
            loss, l2 = m(u, p, n, sample_weight=w) if weighted else m(u, p, n)
        optimizer.apply_gradients(zip(tape.gradient((loss, l2), m.trainable_variables), m.trainable_variables))
        got.append((loss, l2))
        want.append(wr.pair_step("bpr", U, V, b, u, p, n, oo, w=w, l2_reg=0.01))
    assert n_w == 33
    for (loss, l2), (lw, l2w) in zip(got, want):
        assert abs(float(loss) - lw) <= TOL * abs(lw)
        assert abs(float(l2) - 0.01 * l2w) <= TOL * abs(0.01 * l2w)           # the call returns (loss, l2_reg * l2_loss)
    tabs = dict(user=m.user_latent_factor.table, item=m.item_latent_factor.table, bias=m.item_bias.table)
    for r, h in (("user", U), ("item", V), ("bias", b)):
        delta_check(orig[r], tabs[r].read(), h.astype(np.float32), steps=66, what="shim " + r)


def test_queue_never_mixes_weighted_and_unweighted_steps(monkeypatch):
    from openrec_amd import runtime as rt
    from openrec_amd.tf2 import compat as tf
    from openrec_amd.tf2 import recommenders as R
    calls = []
    real = rt.pairwise_step
    monkeypatch.setattr(rt, "pairwise_step", lambda *a, **k: (calls.append((k.get("K"), k.get("weights") is not None, k.get("l2_reg"))), real(*a, **k))[1])
    rng = np.random.default_rng(6)
    m = R.UCML(dim_user_embed=32, dim_item_embed=32, total_users=300, total_items=400, l2_reg=0.5)
    optimizer = tf.keras.optimizers.SGD(0.02)
    for s in range(12):
        u, p, n = (rng.integers(0, 300, 256).astype(np.int32) for _ in range(3))
        w = _weights(rng, 256) if s % 4 < 2 else None
        with tf.GradientTape() as tape:
            out = m(u, p, n, sample_weight=w)
        optimizer.apply_gradients(zip(tape.gradient(out, m.trainable_variables), m.trainable_variables))
    m.flush()
    assert calls == [(2, True, 0.5), (2, False, 0.5)] * 3
    # train_steps: the same keywords in one call
    calls.clear()
    ids = rng.integers(0, 300, (3, 2, 256)).astype(np.int32)
    loss, l2 = m.train_steps(optimizer, ids[0], ids[1], ids[2], sample_weight=_weights(rng, (2, 256)))
    assert calls == [(2, True, 0.5)] and loss.shape == (2,)
