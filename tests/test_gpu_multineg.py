"""GPU: one positive against N negatives (`rt.multineg_step`, `rt.multineg_loss`, `DeviceSampler.pairwise_multi`,
`BPR.train_steps_multi`) against tests/multineg_ref.py in float64, rounded to float32 once.  The cases are
tests/multineg_cases.py's, whose bounds tests/test_multineg_cpu.py proves to leave room for a correct fp32 implementation.
Tolerances are the project's: conftest.delta_check on tables, TOL on loss and l2, TOL_ADAM on Adam's tables."""
import os

import numpy as np
import pytest

import hardneg_ref as hr
import multineg_cases as mc
import multineg_ref as mr
import proposal_ref as pr
from conftest import TOL, TOL_ADAM, delta_check, rel_err

pytestmark = pytest.mark.gpu

DUP = dict(kind="softmax", opt="sgd", bias=True, K=1, B=65, N=5, D=64, NU=30, NI=40, seed=77)      # the duplicate-heavy shape


def _rt():
    from openrec_amd import runtime as rt
    return rt


def _dev_opt(rt, name, ctx=None):
    lr = mc.LR[name]
    if name == "sgd":
        return rt.Optimizer.sgd(lr, ctx=ctx)
    if name == "adagrad":
        return rt.Optimizer.adagrad(lr, ctx=ctx)
    if name == "adam":
        return rt.Optimizer.adam(lr, ctx=ctx)
    return rt.Optimizer.momentum(lr, 0.9, True, ctx=ctx)


def _tables(rt, U, V, b, ctx=None):
    return (rt.Table(*U.shape, ctx).write(U), rt.Table(*V.shape, ctx).write(V), rt.Table(*b.shape, ctx).write(b) if b is not None else None)


def _dev(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() if x is not None else None for x in arrays)


def _bits(*tables):
    return [t.read().view(np.int32) for t in tables if t is not None]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _expect(case, U, V, b, uid, pid, nid, w=None, off=None, l2_reg=1.0, oo=None):
    """the float64 reference: -> tables (float64, stepped in place on copies), [(loss, l2)] per step"""
    U, V = U.astype(np.float64), V.astype(np.float64)
    b = b.astype(np.float64) if b is not None else None
    oo = oo or mc.make_opt(case["opt"])
    out = [mr.step(case["kind"], U, V, b, uid[s], pid[s], nid[s], oo, w=None if w is None else w[s], off=None if off is None else off[s],
                   l2_reg=l2_reg) for s in range(case["K"])]
    return U, V, b, out


def _check(what, case, orig, tabs, want, losses, want_losses):
    for name, W0, t, w in zip(("user", "item", "bias"), orig, tabs, want):
        if t is None:
            continue
        got, w32 = t.read(), w.astype(np.float32)
        print(f"{what} {name}: rel err {rel_err(got, w32):.3g}")
        assert np.isfinite(got).all(), (what, name)
        if case["opt"] == "adam":
            assert rel_err(got, w32) <= TOL_ADAM, (what, name)
        else:
            delta_check(W0, got, w32, steps=case["K"], what=f"{what} {name}")
    if losses is not None:
        for s, (lw, l2w) in enumerate(want_losses):
            print(f"{what} step {s}: loss {losses[0][s]:.8g} want {lw:.8g}  l2 {losses[1][s]:.8g} want {l2w:.8g}")
            assert abs(losses[0][s] - lw) <= TOL * abs(lw) and abs(losses[1][s] - l2w) <= TOL * abs(l2w), (what, s)


def _run(case, w=None, off=None, l2_reg=1.0, no_l2=False, device=False, want_loss=True, check=True, scale=mc.SCALE):
    """one K-step call of the case on fresh tables -> (tables, optimizer, losses)"""
    rt = _rt()
    U, V, b, uid, pid, nid = mc.make(case, scale)
    tabs = _tables(rt, U, V, b)
    opt = _dev_opt(rt, case["opt"])
    args = (uid, pid, nid, w, off)
    if device:
        args = _dev(*args)
    kw = dict(no_l2=True) if no_l2 else dict(l2_reg=l2_reg)
    losses = rt.multineg_step(case["kind"], opt, *tabs, args[0], args[1], args[2], K=case["K"], weights=args[3], neg_offset=args[4],
                              want_loss=want_loss, **kw)
    if check:
        eU, eV, eb, want = _expect(case, U, V, b, uid, pid, nid, w, off, 0.0 if no_l2 else l2_reg)
        _check(case.get("name", "case"), case, (U, V, b), tabs, (eU, eV, eb), losses, want)
    return tabs, opt, losses


# ---- both losses x the four optimizers x with / without the bias x K in {1, 3}, one D per branch of the dispatch ----------------
@pytest.mark.parametrize("case", mc.CASES, ids=[c["name"] for c in mc.CASES])
def test_step_matches_the_float64_reference(case):
    _run(case)


@pytest.mark.parametrize("opt", mc.OPTS)
@pytest.mark.parametrize("bias", [True, False])
def test_three_steps_in_one_call_are_three_calls(opt, bias):
    """within delta_check with the bias (its apply adds with atomics); bit for bit without it (the sorted apply), as is a repeat"""
    rt = _rt()
    case = dict(DUP, opt=opt, bias=bias, K=3, kind="softmax" if bias else "logsig")
    U, V, b, uid, pid, nid = mc.make(case)
    one, _, l_one = _run(case, check=False)
    tabs = _tables(rt, U, V, b)
    o = _dev_opt(rt, opt)
    l_three = [rt.multineg_step(case["kind"], o, *tabs, uid[s], pid[s], nid[s]) for s in range(3)]
    assert np.array_equal(l_one[0], np.concatenate([x[0] for x in l_three])) or bias
    if bias:
        for name, W0, a, c in zip(("user", "item", "bias"), (U, V, b), one, tabs):
            if opt == "adam":
                assert rel_err(a.read(), c.read()) <= TOL_ADAM, name
            else:
                delta_check(W0, a.read(), c.read(), steps=3, what=f"{opt} {name}")
    else:
        assert _same(_bits(*one), _bits(*tabs))
        again, _, l_again = _run(case, check=False)
        assert _same(_bits(*one), _bits(*again)) and np.array_equal(l_one[0].view(np.int32), l_again[0].view(np.int32)) \
            and np.array_equal(l_one[1].view(np.int32), l_again[1].view(np.int32))


def _weights(rng, shape):
    w = rng.uniform(0, 2, shape).astype(np.float32)
    w[..., ::5] = 0.0                           # a weight of 0: the sample keeps only its l2 part
    return w


def _offsets(rng, shape, minus_inf):
    off = rng.normal(0, 1, shape).astype(np.float32)
    if minus_inf:
        off[..., 1] = -np.inf
    return off


@pytest.mark.parametrize("kind", mr.KINDS)
@pytest.mark.parametrize("l2_reg", [0.0, 0.01, 1.0])
def test_weights_offsets_and_the_l2_coefficient(kind, l2_reg):
    """weights with exact zeros, offsets with a column of -inf, every coefficient; SGD and Adagrad, with the bias and without"""
    rng = np.random.default_rng(11)
    for opt, bias, D in (("sgd", True, 64), ("adagrad", False, 24), ("sgd", False, 50)):
        case = dict(DUP, kind=kind, opt=opt, bias=bias, K=2, D=D, NU=300, NI=400, name=f"{kind}-{opt}-l2_{l2_reg}-D{D}")
        w = _weights(rng, (2, 65)); off = _offsets(rng, (2, 65, 5), minus_inf=True)
        _run(case, w=w, off=off, l2_reg=l2_reg)
        _run(case, w=w, l2_reg=l2_reg)
        _run(case, off=_offsets(rng, (2, 65, 5), minus_inf=False), l2_reg=l2_reg, device=True)


@pytest.mark.parametrize("kind", mr.KINDS)
def test_no_l2(kind):
    case = dict(DUP, kind=kind, K=2, NU=300, NI=400, name=f"{kind}-no_l2")
    tabs, _, losses = _run(case, no_l2=True)
    tabs0, _, losses0 = _run(case, l2_reg=0.0, check=False)
    assert np.array_equal(losses[0], losses0[0]) and np.array_equal(losses[1], losses0[1])


@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_host_and_device_inputs_give_the_same_tables(opt):
    rng = np.random.default_rng(12)
    case = dict(DUP, opt=opt, bias=False, K=3, NU=300, NI=400)
    w = _weights(rng, (3, 65)); off = _offsets(rng, (3, 65, 5), minus_inf=True)
    host, _, lh = _run(case, w=w, off=off, check=False)
    dev, _, ld = _run(case, w=w, off=off, device=True, check=False)
    assert _same(_bits(*host), _bits(*dev)) and np.array_equal(lh[0], ld[0]) and np.array_equal(lh[1], ld[1])
    # host lists with id_stride > B: every list is packed step by step, the lists of width N too
    rt = _rt()
    U, V, b, uid, pid, nid = mc.make(case)
    S = 80

    def pad(x, fill):
        out = np.full((3, S) + x.shape[2:], fill, x.dtype)
        out[:, :65] = x
        return out

    tabs = _tables(rt, U, V, b)
    lp = rt.multineg_step(case["kind"], _dev_opt(rt, opt), *tabs, pad(uid, 299), pad(pid, 399), pad(nid, 399), K=3, B=65, id_stride=S,
                          weights=pad(w, 7.0), neg_offset=pad(off, 3.0))
    assert _same(_bits(*host), _bits(*tabs)) and np.array_equal(lh[0], lp[0]) and np.array_equal(lh[1], lp[1])


@pytest.mark.parametrize("opt", mc.OPTS)
def test_without_the_losses_the_tables_are_the_same(opt):
    case = dict(DUP, opt=opt, bias=False, K=3, kind="logsig")
    a, _, losses = _run(case, check=False)
    c, _, none = _run(case, want_loss=False, check=False)
    assert none is None and losses is not None and _same(_bits(*a), _bits(*c))


@pytest.mark.parametrize("kind", mr.KINDS)
@pytest.mark.parametrize("D", [64, 50, 4])
def test_the_forward_is_the_steps_loss_bit_for_bit_and_changes_nothing(kind, D):
    rt = _rt()
    rng = np.random.default_rng(13)
    case = dict(DUP, kind=kind, D=D, B=300, N=16, NU=300, NI=400)
    U, V, b, uid, pid, nid = mc.make(case)
    w = _weights(rng, (1, 300)); off = _offsets(rng, (1, 300, 16), minus_inf=True)
    tabs = _tables(rt, U, V, b)
    before = _bits(*tabs)
    fwd = rt.multineg_loss(kind, *tabs, uid[0], pid[0], nid[0], weights=w[0], neg_offset=off[0])
    assert _same(before, _bits(*tabs))
    fwd_dev = rt.multineg_loss(kind, *tabs, *_dev(uid[0], pid[0], nid[0]), weights=_dev(w[0])[0], neg_offset=_dev(off[0])[0])
    loss, l2 = rt.multineg_step(kind, _dev_opt(rt, "sgd"), *tabs, uid, pid, nid, weights=w, neg_offset=off)
    assert np.float32(fwd[0]).view(np.int32) == loss.view(np.int32)[0] and np.float32(fwd[1]).view(np.int32) == l2.view(np.int32)[0]
    assert fwd_dev == fwd
    want = mr.forward(kind, U.astype(np.float64), V.astype(np.float64), b.astype(np.float64), uid[0], pid[0], nid[0], w[0], off[0])
    assert abs(fwd[0] - want[0]) <= TOL * abs(want[0]) and abs(fwd[1] - want[1]) <= TOL * abs(want[1])


@pytest.mark.parametrize("kind", mr.KINDS)
@pytest.mark.parametrize("D", [64, 50])
def test_large_logits_stay_finite(kind, D):
    """tables scaled until |score| reaches about 200"""
    case = dict(DUP, kind=kind, D=D, N=16, NU=300, NI=400, name=f"{kind}-large-D{D}")
    scale = 5.0 * np.sqrt(64.0 / D)
    U, V, b, uid, pid, nid = mc.make(case, scale)
    top = np.abs(np.einsum("bd,bnd->bn", U[uid[0]].astype(np.float64), V[nid[0]].astype(np.float64))).max()
    print(f"{kind} D={D}: max |score| {top:.1f}")
    assert top >= 150.0
    # (the tables are held to finiteness only: an fp32 score of magnitude 200 carries an absolute error of 1e-5, which is the
    # relative error of every exp(s_j - lse) -- no bound on the update follows from the formats at this scale)
    tabs, _, losses = _run(case, scale=scale, l2_reg=0.01, check=False)
    want = mr.forward(kind, U.astype(np.float64), V.astype(np.float64), b.astype(np.float64), uid[0], pid[0], nid[0])
    print(f"{kind} D={D}: loss {losses[0][0]:.8g} want {want[0]:.8g}  l2 {losses[1][0]:.8g} want {want[1]:.8g}")
    assert np.isfinite(losses[0]).all() and all(np.isfinite(t.read()).all() for t in tabs)
    assert abs(losses[0][0] - want[0]) <= TOL * abs(want[0]) and abs(losses[1][0] - want[1]) <= TOL * abs(want[1])


def test_lazy_adam_a_pairwise_step_then_this_step_then_a_read():
    from oracle import numpy_oracle as orc
    rt = _rt()
    case = dict(DUP, opt="adam", NU=300, NI=400, K=2)
    U, V, b, uid, pid, nid = mc.make(case)
    tabs = _tables(rt, U, V, b)
    opt = _dev_opt(rt, "adam")
    oo = mc.make_opt("adam")
    eU, eV, eb = (x.astype(np.float64) for x in (U, V, b))
    rt.pairwise_step("bpr", opt, *tabs, uid[0], pid[0], nid[0, :, 0])
    orc.bpr_step(eU, eV, eb, uid[0], pid[0], nid[0, :, 0], oo)
    loss, l2 = rt.multineg_step("softmax", opt, *tabs, uid[1], pid[1], nid[1])
    wl, wl2 = mr.step("softmax", eU, eV, eb, uid[1], pid[1], nid[1], oo)
    rt.pairwise_step("bpr", opt, *tabs, uid[0], pid[0], nid[0, :, 1])
    orc.bpr_step(eU, eV, eb, uid[0], pid[0], nid[0, :, 1], oo)
    assert opt.step == 3
    assert abs(loss[0] - wl) <= TOL * abs(wl) and abs(l2[0] - wl2) <= TOL * abs(wl2)
    for name, t, w in zip(("user", "item", "bias"), tabs, (eU, eV, eb)):
        e = rel_err(t.read(), w.astype(np.float32))
        print(f"lazy adam {name}: rel err {e:.3g}")
        assert e <= TOL_ADAM, name


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def _raw_step(rt, ctx, kind, opt, U, V, b, uid, pid, nid, N, l2_reg=1.0, flags=0, K=1):
    from openrec_amd import _ffi
    B = len(uid) // K
    _ffi.check(ctx._lib.orx_multineg_step(ctx._h, kind, opt._h, U._h, V._h, b._h if b is not None else None, uid.ctypes.data,
                                          pid.ctypes.data, nid.ctypes.data, None, None, K, B, N, B, l2_reg, flags, None, None))


def test_bad_arguments_are_refused_before_any_device_work():
    from openrec_amd import _ffi
    rt = _rt()
    U, V, b, uid, pid, nid = mc.make(DUP)
    tabs = _tables(rt, U, V, b)
    ctx = tabs[0].ctx
    before = _bits(*tabs)
    uid, pid, nid = uid[0], pid[0], nid[0]
    sgd = _dev_opt(rt, "sgd")
    other = rt.Context(0)
    base = dict(kind=0, opt=sgd, U=tabs[0], V=tabs[1], b=tabs[2], N=5, l2_reg=1.0, flags=0)
    bad = [dict(N=0), dict(N=65), dict(N=-1), dict(kind=2), dict(kind=-1), dict(flags=_ffi.ORX_HOGWILD), dict(flags=_ffi.ORX_CENSOR),
           dict(l2_reg=-0.5), dict(l2_reg=float("nan")), dict(l2_reg=float("inf")), dict(l2_reg=0.5, flags=_ffi.ORX_NO_L2),
           dict(U=rt.Table(30, 32)), dict(b=rt.Table(40, 2)), dict(b=rt.Table(39, 1)), dict(U=rt.Table(30, 64, other)),
           dict(b=rt.Table(40, 1, other)), dict(opt=_dev_opt(rt, "sgd", other))]
    for kw in bad:
        a = {**base, **kw}
        with pytest.raises(ValueError):
            _raw_step(rt, ctx, a["kind"], a["opt"], a["U"], a["V"], a["b"], uid, pid, nid, a["N"], a["l2_reg"], a["flags"])
    # what orx_apply_rows refuses: the whole-table-sweep form of Adam with a bias column
    os.environ["ORX_ADAM_DENSE"] = "1"
    try:
        with pytest.raises(ValueError, match="ORX_ADAM_DENSE"):
            _raw_step(rt, ctx, 0, _dev_opt(rt, "adam"), *tabs, uid, pid, nid, 5)
    finally:
        del os.environ["ORX_ADAM_DENSE"]
    ctx.synchronize()
    assert _same(before, _bits(*tabs))
    # nothing to do: ORX_OK, nothing launched
    _ffi.check(ctx._lib.orx_multineg_step(ctx._h, 0, sgd._h, tabs[0]._h, tabs[1]._h, tabs[2]._h, None, None, None, None, None,
                                          0, 65, 5, 65, 1.0, 0, None, None))
    _ffi.check(ctx._lib.orx_multineg_step(ctx._h, 0, sgd._h, tabs[0]._h, tabs[1]._h, tabs[2]._h, None, None, None, None, None,
                                          3, 0, 5, 0, 1.0, 0, None, None))
    assert _same(before, _bits(*tabs))
    with pytest.raises(ValueError):
        rt.multineg_loss("softmax", *tabs, uid, pid, np.zeros((65, 65), np.int32))
    from openrec_amd.tf2.recommenders import UCML
    with pytest.raises(NotImplementedError, match="dot products"):
        UCML(8, 8, 10, 10).train_steps_multi(sgd, uid, pid, nid)


@pytest.mark.parametrize("D", [64, 50])
def test_an_id_out_of_range_raises_and_the_context_stays_usable(D):
    """the kernel's own bounds check, on a negative, a positive and a user; then the same call with good ids succeeds"""
    rt = _rt()
    case = dict(DUP, bias=False, D=D, name=f"after-index-error-D{D}")
    U, V, b, uid, pid, nid = mc.make(case)
    for which in range(3):
        tabs = _tables(rt, U, V, b)
        u, p, n = uid.copy(), pid.copy(), nid.copy()
        if which == 0:
            n[0, 17, 3] = case["NI"] + 3
        elif which == 1:
            p[0, 64] = case["NI"]
        else:
            u[0, 0] = case["NU"]
        with pytest.raises(IndexError):
            rt.multineg_step("softmax", _dev_opt(rt, "sgd"), *tabs, u, p, n)
        assert all(np.isfinite(t.read()).all() for t in tabs if t is not None)
    _run(case)


# ---- the sampler ------------------------------------------------------------------------------------------------------------------
SNU, SNI, SNR, SN, SFIRST, SSEED = 500, 300, 7001, 3001, 6000, 7


def _multi(sm, M, first=SFIRST, n=SN, seed=SSEED):
    import torch
    dev = torch.device("cuda", 0)
    u, p = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    ng = torch.full((n, M), -1, dtype=torch.int32, device=dev)
    sm.pairwise_multi(seed, first, n, u, p, ng, negatives=M)
    sm.ctx.synchronize()
    return u.cpu().numpy(), p.cpu().numpy(), ng.cpu().numpy()


@pytest.mark.parametrize("proposal", [False, True])
def test_the_sampler_delivers_the_candidate_stream(proposal):
    import torch
    rt = _rt()
    raw = hr.make_data(0, SNU, SNI, SNR)
    sm = rt.DeviceSampler(raw, SNU, SNI)
    g = np.arange(SFIRST, SFIRST + SN)
    if proposal:
        sm.set_proposal(np.random.default_rng(3).uniform(0.0, 1.0, SNI) ** 3)
        thr, alias = sm.proposal()
        ru, rp, rc = pr.candidates(raw, SNI, SSEED, g, 64, thr, alias)
    else:
        ru, rp, rc = hr.candidates(raw, SNI, SSEED, g, 64)
    dev = torch.device("cuda", 0)
    U = rt.Table(SNU, 16).init_uniform(seed=1); V = rt.Table(SNI, 16).init_uniform(seed=2)
    out = {}
    for M in (1, 5, 16, 64):
        u, p, ng = out[M] = _multi(sm, M)
        assert np.array_equal(u, ru) and np.array_equal(p, rp) and np.array_equal(ng, rc[:, :M]), M
        hu, hp, hn = (torch.empty(SN, dtype=torch.int32, device=dev) for _ in range(3))
        hc = torch.empty(SN * M, dtype=torch.int32, device=dev)
        sm.pairwise_hard(SSEED, SFIRST, SN, hu, hp, hn, "bpr", U, V, None, candidates=M, cand_out=hc)
        sm.ctx.synchronize()
        assert np.array_equal(hc.cpu().numpy().reshape(SN, M), ng) and np.array_equal(hu.cpu().numpy(), u) and np.array_equal(hp.cpu().numpy(), p)
    u0, p0, n0 = (torch.empty(SN, dtype=torch.int32, device=dev) for _ in range(3))
    sm.pairwise(SSEED, SFIRST, SN, u0, p0, n0); sm.ctx.synchronize()
    assert np.array_equal(out[1][2][:, 0], n0.cpu().numpy()) and np.array_equal(out[1][0], u0.cpu().numpy()) and np.array_equal(out[1][1], p0.cpu().numpy())
    # a window does not depend on how it is split into calls
    parts = [_multi(sm, 5, first=SFIRST + a, n=c) for a, c in ((0, 1), (1, 999), (1000, 2001))]
    for k in range(3):
        assert np.array_equal(np.concatenate([x[k] for x in parts]), out[5][k]), k
    with pytest.raises(ValueError):
        sm.pairwise_multi(SSEED, 0, 4, u0, p0, n0, negatives=65)


def test_bpr_train_steps_multi_is_the_runtime_call():
    rt = _rt()
    from openrec_amd.tf2.recommenders import BPR
    rng = np.random.default_rng(14)
    case = dict(DUP, K=3, bias=False)
    U, V, _, uid, pid, nid = mc.make(case)
    w = _weights(rng, (3, 65)); off = _offsets(rng, (3, 65, 5), minus_inf=True)
    for kind in mr.KINDS:
        model = BPR(64, 64, case["NU"], case["NI"], use_item_bias=False, l2_reg=0.01)
        model.user_latent_factor.table.write(U); model.item_latent_factor.table.write(V)
        got = model.train_steps_multi(_dev_opt(rt, "adagrad"), uid, pid, nid, loss=kind, sample_weight=w, neg_offset=off)
        tabs = _tables(rt, U, V, None)
        want = rt.multineg_step(kind, _dev_opt(rt, "adagrad"), *tabs, uid, pid, nid, K=3, weights=w, neg_offset=off, l2_reg=0.01)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert _same(_bits(model.user_latent_factor.table, model.item_latent_factor.table), _bits(*tabs))
