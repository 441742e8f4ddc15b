"""GPU: training on in-batch negatives (`rt.inbatch_step`, `rt.inbatch_loss`, `BPR.train_steps_inbatch`) against
tests/inbatch_ref.py in float64, rounded to float32 once.  The cases are tests/inbatch_cases.py's; the per-row bound is
inbatch_ref.row_bound, whose headroom tests/test_inbatch_cpu.py proves.  Tolerances are the project's: conftest.delta_check on
tables, TOL on loss and l2, TOL_ADAM on Adam's tables."""
import os

import numpy as np
import pytest

import inbatch_cases as ic
import inbatch_ref as ir
from conftest import TOL, TOL_ADAM, delta_check, rel_err

pytestmark = pytest.mark.gpu

DUP = dict(opt="sgd", bias=True, K=1, mask=True, B=65, D=64, NU=30, NI=40, chunk=0, seed=77)      # the duplicate-heavy shape


def _rt():
    from openrec_amd import runtime as rt
    return rt


def _dev_opt(rt, name, ctx=None):
    lr = ic.LR[name]
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


def _same_losses(a, b):
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


def _f64(x):
    return None if x is None else x.astype(np.float64)


def _expect(case, U, V, b, uid, pid, w=None, off=None, scale=1.0, l2_reg=1.0, oo=None):
    """the float64 reference: -> tables (float64, stepped in place on copies), [(loss, l2)] per step"""
    U, V, b = _f64(U), _f64(V), _f64(b)
    oo = oo or ic.make_opt(case["opt"])
    out = [ir.step(U, V, b, uid[s], pid[s], oo, w=None if w is None else _f64(w[s]), off=None if off is None else _f64(off[s]),
                   scale=scale, mask_hits=case["mask"], l2_reg=l2_reg) for s in range(len(uid))]
    return U, V, b, out


def _check(what, case, orig, tabs, want, losses, want_losses, steps):
    for name, W0, t, w in zip(("user", "item", "bias"), orig, tabs, want):
        if t is None:
            continue
        got, w32 = t.read(), w.astype(np.float32)
        print(f"{what} {name}: rel err {rel_err(got, w32):.3g}")
        assert np.isfinite(got).all(), (what, name)
        if case["opt"] == "adam":
            assert rel_err(got, w32) <= TOL_ADAM, (what, name)
        else:
            delta_check(W0, got, w32, steps=steps, what=f"{what} {name}")
    if losses is not None:
        for s, (lw, l2w) in enumerate(want_losses):
            print(f"{what} step {s}: loss {losses[0][s]:.8g} want {lw:.8g}  l2 {losses[1][s]:.8g} want {l2w:.8g}")
            assert abs(losses[0][s] - lw) <= TOL * abs(lw) and abs(losses[1][s] - l2w) <= TOL * abs(l2w), (what, s)


def _run(case, w=None, off=None, scale=1.0, l2_reg=1.0, no_l2=False, device=False, want_loss=True, check=True, tscale=ic.SCALE,
         ids=None):
    """one K-step call of the case on fresh tables -> (tables, optimizer, losses); ids: (uid, pid) in place of the case's own"""
    rt = _rt()
    U, V, b, uid, pid = ic.make(case, tscale)
    if ids is not None:
        uid, pid = ids
    tabs = _tables(rt, U, V, b)
    opt = _dev_opt(rt, case["opt"])
    args = (uid, pid, w, off)
    if device:
        args = _dev(*args)
    kw = dict(no_l2=True) if no_l2 else dict(l2_reg=l2_reg)
    losses = rt.inbatch_step(opt, *tabs, args[0], args[1], K=case["K"], weights=args[2], item_offset=args[3], scale=scale,
                             mask_hits=case["mask"], want_loss=want_loss, chunk=case["chunk"], **kw)
    if check:
        eU, eV, eb, want = _expect(case, U, V, b, uid, pid, w, off, scale, 0.0 if no_l2 else l2_reg)
        _check(case.get("name", "case"), case, (U, V, b), tabs, (eU, eV, eb), losses, want, case["K"])
    return tabs, opt, losses


def _weights(rng, shape):
    w = rng.uniform(0, 2, shape).astype(np.float32)
    w[..., ::5] = 0.0                           # a weight of 0: the sample keeps only its l2 part
    return w


def _offsets(rng, shape):
    return rng.normal(0, 1, shape).astype(np.float32)


# ---- the four optimizers x with / without the bias x K in {1, 3} x the mask on / off, every shape per optimizer --------------------
@pytest.mark.parametrize("case", ic.CASES, ids=[c["name"] for c in ic.CASES])
def test_step_matches_the_float64_reference(case):
    _run(case)


ROW_SHAPES = [si for si, s in enumerate(ic.SHAPES) if s[0] >= 15]


@pytest.mark.parametrize("si", ROW_SHAPES)
@pytest.mark.parametrize("bias,offset,mask", [(True, True, True), (False, False, False), (True, False, False), (False, True, True)])
def test_every_row_loss_is_within_the_bound(si, bias, offset, mask):
    rt = _rt()
    B, D, NU, NI, chunk = ic.SHAPES[si]
    case = dict(opt="sgd", bias=bias, K=1, mask=mask, B=B, D=D, NU=NU, NI=NI, chunk=chunk, seed=500 + si)
    U, V, b, uid, pid = ic.make(case)
    off = _offsets(np.random.default_rng(21 + si), B) if offset else None
    tabs = _tables(rt, U, V, b)
    for scale in (1.0, 4.0):
        loss, l2, rows = rt.inbatch_loss(*tabs, uid[0], pid[0], item_offset=off, scale=scale, mask_hits=mask, chunk=chunk, per_row=True)
        want = ir.row_losses(_f64(U), _f64(V), _f64(b), uid[0], pid[0], _f64(off), scale, mask)
        bound = ir.row_bound(U, V, b, uid[0], pid[0], off, scale, mask)
        err = np.abs(rows.astype(np.float64) - want)
        print(f"B={B} D={D} scale={scale}: worst row {(err / bound).max():.3g} x bound; bound {bound.min():.3g} .. {bound.max():.3g}")
        assert rows.shape == (B,) and np.isfinite(rows).all()
        assert (err <= bound).all(), (int((err > bound).sum()), float((err / bound).max()))
        assert abs(loss - want.mean()) <= TOL * abs(want.mean())


@pytest.mark.parametrize("si", [3, 4, 7])
def test_the_forward_is_the_steps_loss_bit_for_bit_and_changes_nothing(si):
    rt = _rt()
    rng = np.random.default_rng(13)
    B, D, NU, NI, chunk = ic.SHAPES[si]
    case = dict(DUP, B=B, D=D, NU=NU, NI=NI, chunk=chunk)
    U, V, b, uid, pid = ic.make(case)
    w = _weights(rng, (1, B)); off = _offsets(rng, (1, B))
    tabs = _tables(rt, U, V, b)
    before = _bits(*tabs)
    fwd = rt.inbatch_loss(*tabs, uid[0], pid[0], weights=w[0], item_offset=off[0], scale=2.0, chunk=chunk, per_row=True)
    assert _same(before, _bits(*tabs))
    du, dp, dw, do = _dev(uid[0], pid[0], w[0], off[0])
    fwd_dev = rt.inbatch_loss(*tabs, du, dp, weights=dw, item_offset=do, scale=2.0, chunk=chunk, per_row=True)
    loss, l2 = rt.inbatch_step(_dev_opt(rt, "sgd"), *tabs, uid, pid, weights=w, item_offset=off, scale=2.0, chunk=chunk)
    assert np.float32(fwd[0]).view(np.int32) == loss.view(np.int32)[0] and np.float32(fwd[1]).view(np.int32) == l2.view(np.int32)[0]
    assert fwd_dev[:2] == fwd[:2] and np.array_equal(fwd_dev[2].view(np.int32), fwd[2].view(np.int32))
    want = ir.forward(_f64(U), _f64(V), _f64(b), uid[0], pid[0], _f64(w[0]), _f64(off[0]), 2.0, True)
    assert abs(fwd[0] - want[0]) <= TOL * abs(want[0]) and abs(fwd[1] - want[1]) <= TOL * abs(want[1])


@pytest.mark.parametrize("opt", ic.OPTS)
@pytest.mark.parametrize("bias", [True, False])
def test_three_steps_in_one_call_are_three_calls(opt, bias):
    """Losses bit for bit always; tables bit for bit without the bias (the sorted apply), within delta_check with it.  The same
    call twice gives the same bits.  With the bias orx_apply_rows adds every occurrence of an item with an atomic, in an order
    that differs from run to run, so the tables after a step with a REPEATED item are not repeatable and neither is any later
    loss: the case with the bias draws every step's items without repetition (users still repeat), which leaves one add per
    address."""
    rt = _rt()
    case = dict(DUP, opt=opt, bias=bias, K=3, B=130, D=50, NU=200, NI=300, chunk=64)
    U, V, b, uid, pid = ic.make(case)
    if bias:
        rng = np.random.default_rng(31)
        pid = np.stack([rng.permutation(300)[:130] for _ in range(3)]).astype(np.int32)
    one, _, l_one = _run(case, check=False, ids=(uid, pid))
    tabs = _tables(rt, U, V, b)
    o = _dev_opt(rt, opt)
    l_three = [rt.inbatch_step(o, *tabs, uid[s], pid[s], chunk=64) for s in range(3)]
    again, _, l_again = _run(case, check=False, ids=(uid, pid))
    assert _same_losses(l_one, l_again)
    assert _same_losses(l_one, (np.concatenate([x[0] for x in l_three]), np.concatenate([x[1] for x in l_three])))
    if bias:
        for name, W0, a, c in zip(("user", "item", "bias"), (U, V, b), one, tabs):
            if opt == "adam":
                assert rel_err(a.read(), c.read()) <= TOL_ADAM, name
            else:
                delta_check(W0, a.read(), c.read(), steps=3, what=f"{opt} {name}")
    else:
        assert _same(_bits(*one), _bits(*tabs)) and _same(_bits(*one), _bits(*again))


@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_host_and_device_inputs_give_the_same_bits(opt):
    rng = np.random.default_rng(12)
    case = dict(DUP, opt=opt, bias=False, K=3, NU=300, NI=400)
    w = _weights(rng, (3, 65)); off = _offsets(rng, (3, 65))
    host, _, lh = _run(case, w=w, off=off, check=False)
    dev, _, ld = _run(case, w=w, off=off, device=True, check=False)
    assert _same(_bits(*host), _bits(*dev)) and _same_losses(lh, ld)


@pytest.mark.parametrize("opt", ic.OPTS)
def test_without_the_losses_the_tables_are_the_same(opt):
    case = dict(DUP, opt=opt, bias=False, K=3)
    a, _, losses = _run(case, check=False)
    c, _, none = _run(case, want_loss=False, check=False)
    assert none is None and losses is not None and _same(_bits(*a), _bits(*c))


@pytest.mark.parametrize("scale", [0.5, 4.0])
@pytest.mark.parametrize("l2_reg", [0.0, 0.01])
def test_weights_offsets_the_scale_and_the_l2_coefficient(scale, l2_reg):
    """weights with exact zeros, offsets, every coefficient; SGD and Adagrad, with the bias and without, chunked and not"""
    rng = np.random.default_rng(11)
    for opt, bias, B, D, chunk in (("sgd", True, 65, 64, 0), ("adagrad", False, 130, 24, 64), ("sgd", False, 65, 50, 0)):
        case = dict(DUP, opt=opt, bias=bias, K=2, B=B, D=D, NU=300, NI=400, chunk=chunk, name=f"{opt}-scale{scale}-l2_{l2_reg}-D{D}")
        w = _weights(rng, (2, B)); off = _offsets(rng, (2, B))
        _run(case, w=w, off=off, scale=scale, l2_reg=l2_reg)
        _run(case, w=w, scale=scale, l2_reg=l2_reg)
        _run(case, off=off, scale=scale, l2_reg=l2_reg, device=True)


def test_no_l2():
    case = dict(DUP, K=2, NU=300, NI=400, name="no_l2")
    tabs, _, losses = _run(case, no_l2=True)
    tabs0, _, losses0 = _run(case, l2_reg=0.0, check=False)
    assert _same_losses(losses, losses0)


def test_the_mask_on_against_off_on_the_duplicate_heavy_case():
    case = dict(DUP, bias=False, K=2, name="dup-mask")
    on, _, l_on = _run(case)
    off, _, l_off = _run(dict(case, mask=False, name="dup-nomask"))
    assert not _same(_bits(*on), _bits(*off)) and abs(l_on[0][0] - l_off[0][0]) > 1e-3 * abs(l_off[0][0])


@pytest.mark.parametrize("D", [64, 50])
def test_large_logits_stay_finite(D):
    """tables scaled until |score| reaches 150 and beyond"""
    case = dict(DUP, D=D, NU=300, NI=400, name=f"large-D{D}")
    tscale = 5.0 * np.sqrt(64.0 / D)
    U, V, b, uid, pid = ic.make(case, tscale)
    _, _, s = ir.scores(_f64(U), _f64(V), _f64(b), uid[0], pid[0])
    print(f"D={D}: max |s| {np.abs(s).max():.1f}")
    assert np.abs(s).max() >= 150.0
    # (the tables are held to finiteness only: an fp32 score of magnitude 200 carries an absolute error of 1e-5, which is the
    # relative error of every exp(s_ij - lse_i) -- no bound on the update follows from the formats at this scale)
    tabs, _, losses = _run(case, tscale=tscale, l2_reg=0.01, check=False)
    want = ir.forward(_f64(U), _f64(V), _f64(b), uid[0], pid[0])
    print(f"D={D}: loss {losses[0][0]:.8g} want {want[0]:.8g}  l2 {losses[1][0]:.8g} want {want[1]:.8g}")
    assert np.isfinite(losses[0]).all() and all(np.isfinite(t.read()).all() for t in tabs)
    assert abs(losses[0][0] - want[0]) <= TOL * abs(want[0]) and abs(losses[1][0] - want[1]) <= TOL * abs(want[1])


def test_lazy_adam_a_pairwise_step_then_this_step_then_a_read():
    from oracle import numpy_oracle as orc
    rt = _rt()
    case = dict(DUP, opt="adam", NU=300, NI=400, K=2)
    U, V, b, uid, pid = ic.make(case)
    nid = np.random.default_rng(5).integers(0, 400, (2, 65)).astype(np.int32)
    tabs = _tables(rt, U, V, b)
    opt = _dev_opt(rt, "adam")
    oo = ic.make_opt("adam")
    eU, eV, eb = (x.astype(np.float64) for x in (U, V, b))
    rt.pairwise_step("bpr", opt, *tabs, uid[0], pid[0], nid[0])
    orc.bpr_step(eU, eV, eb, uid[0], pid[0], nid[0], oo)
    loss, l2 = rt.inbatch_step(opt, *tabs, uid[1], pid[1])
    wl, wl2 = ir.step(eU, eV, eb, uid[1], pid[1], oo)
    rt.pairwise_step("bpr", opt, *tabs, uid[0], pid[0], nid[1])
    orc.bpr_step(eU, eV, eb, uid[0], pid[0], nid[1], oo)
    assert opt.step == 3
    assert abs(loss[0] - wl) <= TOL * abs(wl) and abs(l2[0] - wl2) <= TOL * abs(wl2)
    for name, t, w in zip(("user", "item", "bias"), tabs, (eU, eV, eb)):
        e = rel_err(t.read(), w.astype(np.float32))
        print(f"lazy adam {name}: rel err {e:.3g}")
        assert e <= TOL_ADAM, name


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def _raw_step(ctx, opt, U, V, b, uid, pid, scale=1.0, l2_reg=1.0, chunk=0, flags=0, K=1):
    from openrec_amd import _ffi
    B = len(uid) // K
    _ffi.check(ctx._lib.orx_inbatch_step(ctx._h, opt._h, U._h, V._h, b._h if b is not None else None, uid.ctypes.data,
                                         pid.ctypes.data, None, None, K, B, B, scale, l2_reg, chunk, flags, None, None))


def test_bad_arguments_are_refused_before_any_device_work():
    from openrec_amd import _ffi
    rt = _rt()
    U, V, b, uid, pid = ic.make(DUP)
    tabs = _tables(rt, U, V, b)
    ctx = tabs[0].ctx
    before = _bits(*tabs)
    uid, pid = uid[0], pid[0]
    sgd = _dev_opt(rt, "sgd")
    other = rt.Context(0)
    base = dict(opt=sgd, U=tabs[0], V=tabs[1], b=tabs[2], scale=1.0, l2_reg=1.0, chunk=0, flags=0)
    bad = [dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")), dict(scale=float("inf")),
           dict(l2_reg=-0.5), dict(l2_reg=float("nan")), dict(l2_reg=float("inf")), dict(l2_reg=0.5, flags=_ffi.ORX_NO_L2),
           dict(flags=_ffi.ORX_HOGWILD), dict(flags=_ffi.ORX_CENSOR), dict(chunk=-64), dict(chunk=32), dict(chunk=100),
           dict(U=rt.Table(30, 32)), dict(U=rt.Table(30, 260), V=rt.Table(40, 260)), dict(b=rt.Table(40, 2)), dict(b=rt.Table(39, 1)),
           dict(U=rt.Table(30, 64, other)), dict(b=rt.Table(40, 1, other)), dict(opt=_dev_opt(rt, "sgd", other))]
    for kw in bad:
        a = {**base, **kw}
        with pytest.raises(ValueError):
            _raw_step(ctx, a["opt"], a["U"], a["V"], a["b"], uid, pid, a["scale"], a["l2_reg"], a["chunk"], a["flags"])
    # what orx_apply_rows refuses: the whole-table-sweep form of Adam with a bias column
    os.environ["ORX_ADAM_DENSE"] = "1"
    try:
        with pytest.raises(ValueError, match="ORX_ADAM_DENSE"):
            _raw_step(ctx, _dev_opt(rt, "adam"), *tabs, uid, pid)
    finally:
        del os.environ["ORX_ADAM_DENSE"]
    ctx.synchronize()
    assert _same(before, _bits(*tabs))
    # nothing to do: ORX_OK, nothing launched
    for K, B in ((0, 65), (3, 0)):
        _ffi.check(ctx._lib.orx_inbatch_step(ctx._h, sgd._h, tabs[0]._h, tabs[1]._h, tabs[2]._h, None, None, None, None,
                                             K, B, B, 1.0, 1.0, 0, 0, None, None))
    assert _same(before, _bits(*tabs))
    with pytest.raises(ValueError):
        rt.inbatch_loss(*tabs, uid, pid, scale=0.0)
    from openrec_amd.tf2.recommenders import UCML
    with pytest.raises(NotImplementedError, match="dot products"):
        UCML(8, 8, 10, 10).train_steps_inbatch(sgd, uid, pid)


@pytest.mark.parametrize("D", [16, 64])
@pytest.mark.parametrize("which", ["uid", "pid"])
def test_an_id_out_of_range_raises_and_leaves_the_good_samples_alone(D, which):
    """the gather's own bounds check: the call raises, the tables stay finite, the good samples match the reference with the bad
    sample removed (weights (B - 1) / B keep c_i = 1 / B), and the next call succeeds"""
    rt = _rt()
    case = dict(DUP, bias=True, D=D, B=130, NU=200, NI=300, chunk=64, name=f"after-index-error-D{D}")
    U, V, b, uid, pid = ic.make(case)
    tabs = _tables(rt, U, V, b)
    u, p = uid.copy(), pid.copy()
    k = 71
    if which == "uid":
        u[0, k] = case["NU"] + 3
    else:
        p[0, k] = -1
    with pytest.raises(IndexError):
        rt.inbatch_step(_dev_opt(rt, "sgd"), *tabs, u, p, chunk=64)
    assert all(np.isfinite(t.read()).all() for t in tabs)
    keep = np.arange(130) != k
    w = np.full((1, 129), 129.0 / 130.0)
    eU, eV, eb, _ = _expect(case, U, V, b, uid[:, keep], pid[:, keep], w=w)
    for name, W0, t, want in zip(("user", "item", "bias"), (U, V, b), tabs, (eU, eV, eb)):
        delta_check(W0, t.read(), want.astype(np.float32), steps=1, what=f"{which} out of range, {name}")
    with pytest.raises(IndexError):
        rt.inbatch_loss(*tabs, u[0], p[0], chunk=64)
    _run(case)


def test_bpr_train_steps_inbatch_is_the_runtime_call():
    rt = _rt()
    from openrec_amd.tf2.recommenders import BPR
    rng = np.random.default_rng(14)
    case = dict(DUP, K=3, bias=False)
    U, V, _, uid, pid = ic.make(case)
    w = _weights(rng, (3, 65)); off = _offsets(rng, (3, 65))
    model = BPR(64, 64, case["NU"], case["NI"], use_item_bias=False, l2_reg=0.01)
    model.user_latent_factor.table.write(U); model.item_latent_factor.table.write(V)
    got = model.train_steps_inbatch(_dev_opt(rt, "adagrad"), uid, pid, sample_weight=w, item_offset=off, scale=2.0, mask_hits=False)
    tabs = _tables(rt, U, V, None)
    want = rt.inbatch_step(_dev_opt(rt, "adagrad"), *tabs, uid, pid, K=3, weights=w, item_offset=off, scale=2.0, mask_hits=False, l2_reg=0.01)
    assert _same_losses(got, want)
    assert _same(_bits(model.user_latent_factor.table, model.item_latent_factor.table), _bits(*tabs))
