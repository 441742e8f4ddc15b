"""GPU: training on the full softmax over all items (`rt.fullsoftmax_step`, `rt.fullsoftmax_loss`, `rt.SeqRec.step_full`,
`BPR.train_steps_full`, `VanillaYouTubeRec.train_steps_full`) against tests/fullsoftmax_ref.py in float64, rounded to float32
once.  The cases are tests/fullsoftmax_cases.py's; the per-row bound is fullsoftmax_ref.row_bound, whose headroom
tests/test_fullsoftmax_cpu.py shows.  Tolerances are the project's: conftest.delta_check on tables, TOL on loss and l2, TOL_ADAM
on Adam's tables and slots."""
import os

import numpy as np
import pytest

import fullsoftmax_cases as fc
import fullsoftmax_ref as fr
from conftest import TOL, TOL_ADAM, delta_check, rel_err

pytestmark = pytest.mark.gpu

SMALL = dict(opt="sgd", bias=True, B=65, D=64, NU=30, NI=40, chunk_items=0, chunk_samples=64, seed=77, name="small")
MID = dict(opt="sgd", bias=True, B=130, D=50, NU=200, NI=300, chunk_items=128, chunk_samples=64, seed=78, name="mid")


def _rt():
    from openrec_amd import runtime as rt
    return rt


def _dev_opt(rt, name, ctx=None):
    lr = fc.LR[name]
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
    return None if x is None else np.asarray(x).astype(np.float64)


def _weights(rng, n):
    w = rng.uniform(0, 2, n).astype(np.float32)
    w[::5] = 0.0                                # a weight of 0: the sample keeps only its l2 part
    return w


def _offsets(rng, n):
    return rng.normal(0, 1, n).astype(np.float32)


def _check_tables(what, optname, names, orig, got_tabs, want, steps=1):
    for name, W0, t, w in zip(names, orig, got_tabs, want):
        if t is None:
            continue
        got, w32 = t.read(), w.astype(np.float32)
        print(f"{what} {name}: rel err {rel_err(got, w32):.3g}")
        assert np.isfinite(got).all(), (what, name)
        if optname == "adam":
            assert rel_err(got, w32) <= TOL_ADAM, (what, name)
        else:
            delta_check(W0, got, w32, steps=steps, what=f"{what} {name}")


def _check_losses(what, losses, want):
    print(f"{what}: loss {losses[0][0]:.8g} want {want[0]:.8g}  l2 {losses[1][0]:.8g} want {want[1]:.8g}")
    assert abs(losses[0][0] - want[0]) <= TOL * abs(want[0]) and abs(losses[1][0] - want[1]) <= TOL * abs(want[1]), what


def _run(case, w=None, off=None, scale=1.0, l2_reg=0.01, device=False, want_loss=True, check=True, tscale=fc.SCALE, ids=None,
         train=None, chunks=None):
    """one step of the case on fresh tables -> (tables, optimizer, losses, the float64 reference's optimizer)"""
    rt = _rt()
    U, V, b, uid, pid = fc.make(case, tscale)
    if ids is not None:
        uid, pid = ids
    tabs = _tables(rt, U, V, b)
    opt = _dev_opt(rt, case["opt"])
    args = (uid, pid, w, off)
    if device:
        args = _dev(*args)
    ci, cs = (case["chunk_items"], case["chunk_samples"]) if chunks is None else chunks
    losses = rt.fullsoftmax_step(opt, *tabs, args[0], args[1], weights=args[2], item_offset=args[3], scale=scale, l2_reg=l2_reg,
                                 train=train, chunk_items=ci, chunk_samples=cs, want_loss=want_loss)
    oo = None
    if check:
        e = [_f64(U), _f64(V), _f64(b)]
        oo = fc.make_opt(case["opt"])
        want = fr.step(*e, uid, pid, oo, w=_f64(w), off=_f64(off), scale=scale, l2_reg=float(np.float32(l2_reg)),
                       train=train or ("user", "item", "bias"))
        _check_tables(case.get("name", "case"), case["opt"], ("user", "item", "bias"), (U, V, b), tabs, e)
        if losses is not None:
            _check_losses(case.get("name", "case"), losses, want)
        if case["opt"] == "adam":                 # the slots of the dense-applied tables
            for name, t, key in (("item", tabs[1], "V"), ("bias", tabs[2], "b")):
                if t is None or (train is not None and name not in train):
                    continue
                for slot, ref in ((0, oo.m[key]), (1, oo.v[key])):
                    got = np.asarray(opt.slot(t, slot)).reshape(ref.shape)
                    assert rel_err(got, ref.astype(np.float32)) <= TOL_ADAM, (name, slot)
    return tabs, opt, losses, oo


# ---- 1. the four optimizers x with / without the bias, every shape per optimizer ---------------------------------------------------
@pytest.mark.parametrize("case", fc.CASES, ids=[c["name"] for c in fc.CASES])
def test_step_matches_the_float64_reference(case):
    _run(case)


# ---- 2. the row losses -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(fc.SHAPES)))
@pytest.mark.parametrize("bias,offset", [(True, True), (False, False), (True, False), (False, True)])
def test_every_row_loss_is_within_the_bound(si, bias, offset):
    rt = _rt()
    case = fc.shape_case(si, bias=bias, seed=500 + si)
    U, V, b, uid, pid = fc.make(case)
    off = _offsets(np.random.default_rng(21 + si), case["NI"]) if offset else None
    tabs = _tables(rt, U, V, b)
    for scale in (1.0, 4.0):
        loss, l2, rows = rt.fullsoftmax_loss(*tabs, uid, pid, item_offset=off, scale=scale, chunk_items=case["chunk_items"], per_row=True)
        want = fr.row_losses(_f64(U), _f64(V), _f64(b), uid, pid, _f64(off), scale)
        bound = fr.row_bound(U, V, b, uid, pid, off, scale)
        err = np.abs(rows.astype(np.float64) - want)
        print(f"{case['name']} scale={scale}: worst row {(err / bound).max():.3g} x bound; bound {bound.min():.3g} .. {bound.max():.3g}")
        assert rows.shape == (case["B"],) and np.isfinite(rows).all()
        assert (err <= bound).all(), (int((err > bound).sum()), float((err / bound).max()))
        assert abs(loss - want.mean()) <= TOL * abs(want.mean())


def test_items_removed_by_an_offset_of_minus_infinity():
    """a few items at -inf: they are in nobody's softmax (the row losses are those of the table without them), their G_V and G_b
    are exactly 0 beyond the l2 term -- under SGD with l2_reg = 0 their rows and biases keep their bits"""
    rt = _rt()
    case = dict(MID, name="minus-inf")
    U, V, b, uid, pid = fc.make(case)
    rng = np.random.default_rng(3)
    gone = np.setdiff1d(rng.permutation(case["NI"])[:9], pid)[:6]
    assert len(gone) >= 3
    off = _offsets(rng, case["NI"]); off[gone] = -np.inf
    tabs = _tables(rt, U, V, b)
    loss, l2, rows = rt.fullsoftmax_loss(*tabs, uid, pid, item_offset=off, chunk_items=128, per_row=True)
    want = fr.row_losses(_f64(U), _f64(V), _f64(b), uid, pid, _f64(off))
    bound = fr.row_bound(U, V, b, uid, pid, off)
    assert np.isfinite(rows).all() and (np.abs(rows - want) <= bound).all()
    before = _bits(*tabs)
    for device in (False, True):
        tabs, _, losses, _ = _run(case, off=off, l2_reg=0.0, device=device)
        after = _bits(*tabs)
        assert np.array_equal(before[1][gone], after[1][gone]) and np.array_equal(before[2][gone], after[2][gone])
        assert not np.array_equal(before[1], after[1])


# ---- 3. the forward is the step's loss; repeatability ------------------------------------------------------------------------------
@pytest.mark.parametrize("si", [3, 4, 7])
def test_the_forward_is_the_steps_loss_bit_for_bit_and_changes_nothing(si):
    rt = _rt()
    rng = np.random.default_rng(13)
    case = fc.shape_case(si)
    U, V, b, uid, pid = fc.make(case)
    w = _weights(rng, case["B"]); off = _offsets(rng, case["NI"])
    ci, cs = case["chunk_items"], case["chunk_samples"]
    tabs = _tables(rt, U, V, b)
    before = _bits(*tabs)
    fwd = rt.fullsoftmax_loss(*tabs, uid, pid, weights=w, item_offset=off, scale=2.0, chunk_items=ci, per_row=True)
    assert _same(before, _bits(*tabs))
    du, dp, dw, do = _dev(uid, pid, w, off)
    fwd_dev = rt.fullsoftmax_loss(*tabs, du, dp, weights=dw, item_offset=do, scale=2.0, chunk_items=ci, per_row=True)
    loss, l2 = rt.fullsoftmax_step(_dev_opt(rt, "sgd"), *tabs, uid, pid, weights=w, item_offset=off, scale=2.0, chunk_items=ci, chunk_samples=cs)
    assert np.float32(fwd[0]).view(np.int32) == loss.view(np.int32)[0] and np.float32(fwd[1]).view(np.int32) == l2.view(np.int32)[0]
    assert fwd_dev[:2] == fwd[:2] and np.array_equal(fwd_dev[2].view(np.int32), fwd[2].view(np.int32))
    want = fr.forward(_f64(U), _f64(V), _f64(b), uid, pid, _f64(w), _f64(off), 2.0)
    assert abs(fwd[0] - want[0]) <= TOL * abs(want[0]) and abs(fwd[1] - want[1]) <= TOL * abs(want[1])


@pytest.mark.parametrize("opt", fc.OPTS)
def test_two_runs_of_a_step_give_the_same_bits_in_every_table(opt):
    """labels repeat (65 samples over 40 items) and so do users: no sum of the step depends on the run"""
    case = dict(SMALL, opt=opt)
    rng = np.random.default_rng(2)
    w = _weights(rng, 65); off = _offsets(rng, 40)
    a, _, la, _ = _run(case, w=w, off=off, check=False)
    c, _, lc, _ = _run(case, w=w, off=off, check=False)
    assert _same(_bits(*a), _bits(*c)) and _same_losses(la, lc)


# ---- 4. where the inputs live; without the losses ----------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_host_and_device_inputs_give_the_same_bits(opt):
    rng = np.random.default_rng(12)
    case = dict(MID, opt=opt)
    w = _weights(rng, case["B"]); off = _offsets(rng, case["NI"])
    host, _, lh, _ = _run(case, w=w, off=off, check=False)
    dev, _, ld, _ = _run(case, w=w, off=off, device=True, check=False)
    assert _same(_bits(*host), _bits(*dev)) and _same_losses(lh, ld)


@pytest.mark.parametrize("opt", fc.OPTS)
def test_without_the_losses_the_tables_are_the_same(opt):
    case = dict(SMALL, opt=opt)
    a, _, losses, _ = _run(case, check=False)
    c, _, none, _ = _run(case, want_loss=False, check=False, device=True)
    assert none is None and losses is not None and _same(_bits(*a), _bits(*c))


# ---- 5. forced chunking against the launcher's own ---------------------------------------------------------------------------------
def test_forced_chunking_against_the_launchers_own():
    """each is held to the reference; bit equality between the two is not required"""
    case = dict(fc.shape_case(5, "adagrad"), name="chunked")
    assert case["chunk_items"] and case["chunk_samples"]
    _run(case)
    _run(dict(case, name="own-chunking"), chunks=(0, 0))
    _run(dict(case, name="one-tile-chunks"), chunks=(64, 64))


# ---- 6. the coefficients -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0.5, 4.0])
@pytest.mark.parametrize("l2_reg", [0.0, 0.01])
def test_weights_offsets_the_scale_and_the_l2_coefficient(scale, l2_reg):
    rng = np.random.default_rng(11)
    for opt, bias, D in (("sgd", True, 64), ("adagrad", False, 24), ("momentum", True, 50)):
        case = dict(MID, opt=opt, bias=bias, D=D, name=f"{opt}-scale{scale}-l2_{l2_reg}-D{D}")
        w = _weights(rng, case["B"]); off = _offsets(rng, case["NI"])
        _run(case, w=w, off=off, scale=scale, l2_reg=l2_reg)
        _run(case, w=w, scale=scale, l2_reg=l2_reg)
        _run(case, off=off, scale=scale, l2_reg=l2_reg, device=True)


def test_no_l2_is_l2_reg_zero():
    from openrec_amd import _ffi
    rt = _rt()
    U, V, b, uid, pid = fc.make(SMALL)
    tabs = _tables(rt, U, V, b)
    ctx = tabs[0].ctx
    sgd = _dev_opt(rt, "sgd")
    _ffi.check(ctx._lib.orx_fullsoftmax_step(ctx._h, sgd._h, tabs[0]._h, tabs[1]._h, tabs[2]._h, uid.ctypes.data,
                                             pid.ctypes.data, None, None, 65, 1.0, 0.0, 0, 64, 0, _ffi.ORX_NO_L2, None, None))
    zero, _, _, _ = _run(SMALL, l2_reg=0.0)
    assert _same(_bits(*tabs), _bits(*zero))


@pytest.mark.parametrize("D", [4, 256])
def test_large_logits_stay_finite(D):
    """tables scaled until |score| is about 200"""
    case = dict(SMALL, D=D, NU=300, NI=400, name=f"large-D{D}")
    tscale = {4: 9.0, 256: 3.2}[D]
    U, V, b, uid, pid = fc.make(case, tscale)
    s = fr.scores(_f64(U)[uid], _f64(V), _f64(b))
    print(f"D={D}: max |s| {np.abs(s).max():.1f}")
    assert np.abs(s).max() >= 150.0
    # (the tables are held to finiteness only: an fp32 score of magnitude 200 carries an absolute error of 1e-5, which is the
    # relative error of every exp(s_ij - lse_i) -- no bound on the update follows from the formats at this scale)
    tabs, _, losses, _ = _run(case, tscale=tscale, l2_reg=0.01, check=False)
    want = fr.forward(_f64(U), _f64(V), _f64(b), uid, pid)
    print(f"D={D}: loss {losses[0][0]:.8g} want {want[0]:.8g}  l2 {losses[1][0]:.8g} want {want[1]:.8g}")
    assert np.isfinite(losses[0]).all() and all(np.isfinite(t.read()).all() for t in tabs)
    assert abs(losses[0][0] - want[0]) <= TOL * abs(want[0]) and abs(losses[1][0] - want[1]) <= TOL * abs(want[1])


# ---- 7. train masks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_train_masks_leave_the_other_tables_bit_identical(opt):
    rt = _rt()
    case = dict(MID, opt=opt, name=f"mask-{opt}")
    U, V, b, uid, pid = fc.make(case)
    before = [x.view(np.int32) for x in (U, V, b)]
    tabs, o, _, _ = _run(case, train=("user",))
    after = _bits(*tabs)
    assert np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2]) and not np.array_equal(before[0], after[0])
    if opt == "adam":
        assert all(not np.asarray(o.slot(t, s)).any() for t in tabs[1:] for s in (0, 1))
    tabs, o, _, _ = _run(case, train=("item", "bias"))
    after = _bits(*tabs)
    assert np.array_equal(before[0], after[0]) and not np.array_equal(before[1], after[1]) and not np.array_equal(before[2], after[2])
    tabs, o, _, _ = _run(case, train=("item",))
    after = _bits(*tabs)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[2], after[2])


# ---- 8. lazy Adam ------------------------------------------------------------------------------------------------------------------
def test_lazy_adam_a_pairwise_step_then_this_step_then_a_pairwise_step_then_a_read():
    """V and b were finished before the forward and can go back to the sparse steps: one AdamTFSparse state throughout"""
    from oracle import numpy_oracle as orc
    rt = _rt()
    case = dict(MID, opt="adam")
    U, V, b, uid, pid = fc.make(case)
    rng = np.random.default_rng(5)
    uid2, pid2 = rng.integers(0, case["NU"], (2, 130)).astype(np.int32), rng.integers(0, case["NI"], (2, 130)).astype(np.int32)
    nid = rng.integers(0, case["NI"], (2, 130)).astype(np.int32)
    tabs = _tables(rt, U, V, b)
    opt = _dev_opt(rt, "adam")
    oo = fc.make_opt("adam")
    eU, eV, eb = (_f64(x) for x in (U, V, b))
    rt.pairwise_step("bpr", opt, *tabs, uid2[0], pid2[0], nid[0])
    orc.bpr_step(eU, eV, eb, uid2[0], pid2[0], nid[0], oo)
    loss, l2 = rt.fullsoftmax_step(opt, *tabs, uid, pid, l2_reg=0.01, chunk_items=128, chunk_samples=64)
    wl, wl2 = fr.step(eU, eV, eb, uid, pid, oo, l2_reg=float(np.float32(0.01)))
    rt.pairwise_step("bpr", opt, *tabs, uid2[1], pid2[1], nid[1])
    orc.bpr_step(eU, eV, eb, uid2[1], pid2[1], nid[1], oo)
    assert opt.step == 3
    assert abs(loss[0] - wl) <= TOL * abs(wl) and abs(l2[0] - wl2) <= TOL * abs(wl2)
    for name, t, w in zip(("user", "item", "bias"), tabs, (eU, eV, eb)):
        e = rel_err(t.read(), w.astype(np.float32))
        print(f"lazy adam {name}: rel err {e:.3g}")
        assert e <= TOL_ADAM, name


# ---- 9. ids out of range -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [3, 64])
@pytest.mark.parametrize("which", ["uid", "pid"])
def test_an_id_out_of_range_raises_and_leaves_the_good_samples_alone(D, which):
    """the prepare pass's own bounds check: the call raises, the good samples' row losses are those of the call without the bad id
    bit for bit, the tables match the reference with the bad sample removed (weights (B - 1) / B keep c_i = 1 / B), and the
    next call succeeds"""
    rt = _rt()
    case = dict(MID, D=D, name=f"after-index-error-D{D}")
    U, V, b, uid, pid = fc.make(case)
    tabs = _tables(rt, U, V, b)
    good = rt.fullsoftmax_loss(*tabs, uid, pid, chunk_items=128, per_row=True)[2]
    u, p = uid.copy(), pid.copy()
    k = 71
    if which == "uid":
        u[k] = case["NU"] + 3
    else:
        p[k] = -1
    keep = np.arange(130) != k
    import torch
    rows = torch.zeros(130, dtype=torch.float32, device="cuda")
    from openrec_amd import _ffi
    ctx = tabs[0].ctx
    du, dp = _dev(u, p)
    ctx.after_torch(du, dp, rows)
    with pytest.raises(IndexError):
        _ffi.check(ctx._lib.orx_fullsoftmax_loss(ctx._h, tabs[0]._h, tabs[1]._h, tabs[2]._h, du.data_ptr(), dp.data_ptr(), None, None, 130, 1.0,
                                                 128, _ffi.ORX_IDS_DEVICE, None, None, rows.data_ptr()))
    rows = rows.cpu().numpy()
    assert np.array_equal(rows[keep].view(np.int32), good[keep].view(np.int32)) and rows[k] == 0.0
    with pytest.raises(IndexError):
        rt.fullsoftmax_step(_dev_opt(rt, "sgd"), *tabs, u, p, l2_reg=0.01, chunk_items=128, chunk_samples=64)
    assert all(np.isfinite(t.read()).all() for t in tabs)
    w = np.full(129, 129.0 / 130.0)
    e = [_f64(U), _f64(V), _f64(b)]
    fr.step(*e, uid[keep], pid[keep], fc.make_opt("sgd"), w=w, l2_reg=float(np.float32(0.01)))
    _check_tables(f"{which} out of range", "sgd", ("user", "item", "bias"), (U, V, b), tabs, e)
    with pytest.raises(IndexError):
        rt.fullsoftmax_loss(*tabs, u, p, chunk_items=128)
    _run(case)


# ---- 10. the SeqRec route ------------------------------------------------------------------------------------------------------------
def _seq_tables(rt, case):
    rng = np.random.default_rng(case["seed"] + 900)
    _, V, b, _, pid = fc.make(case)
    H = rng.uniform(-fc.SCALE, fc.SCALE, V.shape).astype(np.float32)
    return H, V, b, pid


@pytest.mark.parametrize("pool", ["mean", "sum", ("fixed", 6.0)], ids=["mean", "sum", "fixed"])
@pytest.mark.parametrize("opt", fc.OPTS)
def test_seqrec_step_full_matches_the_composed_reference(pool, opt):
    """ragged bags, one of them empty; host lists, then the padded pair on the device: the ragged form's bits"""
    rt = _rt()
    case = dict(MID, opt=opt, bias=opt != "adagrad", name=f"seq-{opt}")
    H, V, b, pid = _seq_tables(rt, case)
    ptr, items = fc.make_bags(case)
    rng = np.random.default_rng(4)
    w = _weights(rng, case["B"]); off = _offsets(rng, case["NI"])
    tabs = _tables(rt, H, V, b)
    net = rt.SeqRec(*tabs, pool=pool)
    o = _dev_opt(rt, opt)
    fwd = net.loss_full((ptr, items), pid, weights=w, item_offset=off, scale=2.0, chunk_items=128, per_row=True)
    losses = net.step_full(o, (ptr, items), pid, weights=w, item_offset=off, scale=2.0, l2_reg=0.01, chunk_items=128, chunk_samples=64)
    assert np.float32(fwd[0]).view(np.int32) == losses[0].view(np.int32)[0] and np.float32(fwd[1]).view(np.int32) == losses[1].view(np.int32)[0]
    e = [_f64(H), _f64(V), _f64(b)]
    want_rows = fr.seq_row_losses(*e, ptr, items, pid, pool, _f64(off), 2.0)
    want = fr.seq_step(*e, ptr, items, pid, fc.make_opt(opt), pool, w=_f64(w), off=_f64(off), scale=2.0, l2_reg=float(np.float32(0.01)))
    _check_tables(case["name"], opt, ("history", "item", "bias"), (H, V, b), tabs, e)
    _check_losses(case["name"], losses, want)
    assert abs(float(np.mean(_f64(w) * want_rows)) - want[0]) <= 1e-12 * abs(want[0]) and fwd[2].shape == (case["B"],)
    # the padded pair, on the device
    lens = np.diff(ptr)
    seq = np.full((case["B"], int(lens.max()) + 2), -7, np.int32)
    for i, n in enumerate(lens):
        seq[i, :n] = items[ptr[i]:ptr[i + 1]]
    tabs2 = _tables(rt, H, V, b)
    dseq, dlen, dpid, dw, doff = _dev(seq, lens.astype(np.int32), pid, w, off)
    l2nd = rt.SeqRec(*tabs2, pool=pool).step_full(_dev_opt(rt, opt), (dseq, dlen), dpid, weights=dw, item_offset=doff, scale=2.0,
                                                  l2_reg=0.01, chunk_items=128, chunk_samples=64)
    assert _same(_bits(*tabs), _bits(*tabs2)) and _same_losses(losses, l2nd)


def test_seqrec_with_bags_of_one_and_sum_pooling_is_the_user_table_form():
    """H = U, bag i = [uid[i]]: loss and l2 bit for bit; the tables to delta_check (the history route sums in another order)"""
    rt = _rt()
    case = dict(MID, NU=300)
    U, V, b, uid, pid = fc.make(case)
    a = _tables(rt, U, V, b)
    la = rt.fullsoftmax_step(_dev_opt(rt, "sgd"), *a, uid, pid, l2_reg=0.01, chunk_items=128, chunk_samples=64)
    c = _tables(rt, U, V, b)
    ptr = np.arange(131, dtype=np.int32)
    lc = rt.SeqRec(*c, pool="sum").step_full(_dev_opt(rt, "sgd"), (ptr, uid), pid, l2_reg=0.01, chunk_items=128, chunk_samples=64)
    assert _same_losses(la, lc)
    for name, W0, x, y in zip(("user", "item", "bias"), (U, V, b), a, c):
        delta_check(W0, y.read(), x.read(), steps=1, what=f"bags of one, {name}")


def test_seqrec_train_masks_and_bad_lists():
    rt = _rt()
    case = dict(MID, opt="adam", name="seq-mask")
    H, V, b, pid = _seq_tables(rt, case)
    ptr, items = fc.make_bags(case)
    before = [x.view(np.int32) for x in (H, V, b)]
    tabs = _tables(rt, H, V, b)
    net = rt.SeqRec(*tabs)
    net.step_full(_dev_opt(rt, "adam"), (ptr, items), pid, train=("history",))
    after = _bits(*tabs)
    assert np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2]) and not np.array_equal(before[0], after[0])
    tabs = _tables(rt, H, V, b)
    net = rt.SeqRec(*tabs)
    net.step_full(_dev_opt(rt, "adam"), (ptr, items), pid, train=("item", "bias"))
    after = _bits(*tabs)
    assert np.array_equal(before[0], after[0]) and not np.array_equal(before[1], after[1])
    # a bad id inside a bag; a malformed device bag_ptr: IndexError, the good bags' rows unchanged, the context usable
    tabs = _tables(rt, H, V, b)
    net = rt.SeqRec(*tabs)
    good = net.loss_full((ptr, items), pid, chunk_items=128, per_row=True)[2]
    it = items.copy(); it[ptr[3] + 1] = case["NI"]
    with pytest.raises(IndexError):
        net.loss_full((ptr, it), pid, chunk_items=128)
    with pytest.raises(IndexError):
        net.step_full(_dev_opt(rt, "sgd"), (ptr, it), pid)
    dec = ptr.copy(); dec[5] = dec[4] - 1
    with pytest.raises(ValueError):
        net.step_full(_dev_opt(rt, "sgd"), (dec, items), pid)
    with pytest.raises(IndexError):
        net.step_full(_dev_opt(rt, "sgd"), _dev(dec, items), *_dev(pid))
    assert all(np.isfinite(t.read()).all() for t in tabs)
    tabs = _tables(rt, H, V, b)
    again = rt.SeqRec(*tabs).loss_full((ptr, items), pid, chunk_items=128, per_row=True)[2]
    assert np.array_equal(again.view(np.int32), good.view(np.int32))


# ---- 10b. the drivers' two early-outs, on every entry point that goes through them ---------------------------------------------------------
TEN = ("fullsoftmax_step", "fullsoftmax_loss", "seqrec_full_step", "seqrec_full_loss", "seqrec_full_sets_step", "seqrec_full_sets_loss",
       "tower_step", "tower_loss", "tower_sets_step", "tower_sets_loss")


def _tiny_model(rt, entry, seed=5):
    """items = 65, D = 8: -> (the call of `entry` on (opt, bags, B), the tables by name)"""
    rng = np.random.default_rng(seed)
    T = lambda rows, dim: rt.Table(rows, dim).write(rng.uniform(-0.3, 0.3, (rows, dim)).astype(np.float32))
    tabs = dict(V=T(65, 8), b=T(65, 1))
    if entry.startswith("fullsoftmax"):
        tabs["U"] = T(10, 8)
    elif entry.startswith("seqrec"):
        tabs["H"] = T(65, 8)
        net = rt.SeqRec(tabs["H"], tabs["V"], tabs["b"])
    else:
        tabs.update(H=T(65, 6), S0=T(7, 3), W0=T(9, 12), c0=T(1, 12), W1=T(12, 8))
        net = rt.DeepSeqRec(tabs["H"], tabs["V"], tabs["b"], [(tabs["W0"], tabs["c0"]), tabs["W1"]], side=[tabs["S0"]], relu_last=False)

    def call(opt, bags, B):
        ids = rng.integers(0, 7, B).astype(np.int32)
        kw = dict(labels=(np.arange(B + 1, dtype=np.int32), ids)) if "sets" in entry else {}
        if entry.startswith("tower"):
            kw["side_ids"] = (ids,)
        if entry.startswith("fullsoftmax"):
            head = (tabs["U"], tabs["V"], tabs["b"], ids, ids)
            return rt.fullsoftmax_step(opt, *head) if entry.endswith("step") else rt.fullsoftmax_loss(*head, per_row=True)
        pid = None if "sets" in entry else ids
        return net.step_full(opt, bags, pid, **kw) if entry.endswith("step") else net.loss_full(bags, pid, per_row=True, **kw)
    return call, tabs


@pytest.mark.parametrize("entry", TEN)
def test_an_empty_batch_succeeds_and_changes_nothing(entry, monkeypatch):
    rt = _rt()
    call, tabs = _tiny_model(rt, entry)
    before = _bits(*tabs.values())
    made = []

    def outputs(K, want_loss):          # the (loss, l2) pair the library is handed, holding 7 and not 0 beforehand
        out = np.full(K, 7.0, np.float32), np.full(K, 7.0, np.float32)
        made.append(out)
        return out, out[0].ctypes.data, out[1].ctypes.data
    monkeypatch.setattr(rt, "_loss_outputs", outputs)
    got = call(_dev_opt(rt, "adam"), (np.zeros(1, np.int32), np.zeros(0, np.int32)), 0)
    assert len(made) == 1
    if entry.endswith("loss"):          # the forward's early-out writes its zeros
        assert made[0][0][0] == 0.0 and made[0][1][0] == 0.0 and got[:2] == (0.0, 0.0) and got[2].shape == (0,)
    assert _same(before, _bits(*tabs.values()))


@pytest.mark.parametrize("entry", [e for e in TEN if e.endswith("step")])
def test_a_step_without_an_optimizer_is_refused_by_name(entry):
    """the raw C call with opt = NULL: the step's own checks refuse it, whatever else the call holds; no table changes"""
    rt = _rt()
    call, tabs = _tiny_model(rt, entry)
    before = _bits(*tabs.values())

    class NoOptimizer:
        _h, _tables = None, []
    with pytest.raises(ValueError, match="orx_" + entry + ": NULL optimizer"):
        call(NoOptimizer(), (np.arange(6, dtype=np.int32), np.arange(5, dtype=np.int32)), 5)
    assert _same(before, _bits(*tabs.values()))


@pytest.mark.parametrize("opt", ["sgd", "adam"])
@pytest.mark.parametrize("entry", [e for e in TEN if e.endswith("step") and not e.startswith("fullsoftmax")])
def test_every_bag_empty_with_the_history_trained_moves_the_item_side_alone(entry, opt):
    rt = _rt()
    call, tabs = _tiny_model(rt, entry)
    before = {k: t.read().view(np.int32) for k, t in tabs.items()}
    losses = call(_dev_opt(rt, opt), (np.zeros(6, np.int32), np.zeros(0, np.int32)), 5)
    after = {k: t.read().view(np.int32) for k, t in tabs.items()}
    assert np.isfinite(losses[0]).all() and np.isfinite(losses[1]).all()
    assert np.array_equal(before["H"], after["H"])
    # the item side moves: the bias always; the item rows where the query is not 0 (SeqRec pools an empty bag to q = 0, so g_V = 0;
    # the tower's query comes from the side rows and the layers' biases)
    assert not np.array_equal(before["b"], after["b"])
    assert np.array_equal(before["V"], after["V"]) == entry.startswith("seqrec")


# ---- 11. refusals --------------------------------------------------------------------------------------------------------------------
def _raw_step(ctx, opt, U, V, b, uid, pid, scale=1.0, l2_reg=0.0, ci=0, cs=0, mask=0, flags=0):
    from openrec_amd import _ffi
    _ffi.check(ctx._lib.orx_fullsoftmax_step(ctx._h, opt._h, U._h, V._h, b._h if b is not None else None, uid.ctypes.data,
                                             pid.ctypes.data, None, None, len(uid), scale, l2_reg, ci, cs, mask, flags, None, None))


def test_bad_arguments_are_refused_before_any_device_work():
    from openrec_amd import _ffi
    rt = _rt()
    U, V, b, uid, pid = fc.make(SMALL)
    tabs = _tables(rt, U, V, b)
    ctx = tabs[0].ctx
    before = _bits(*tabs)
    sgd = _dev_opt(rt, "sgd")
    other = rt.Context(0)
    base = dict(opt=sgd, U=tabs[0], V=tabs[1], b=tabs[2], scale=1.0, l2_reg=0.0, ci=0, cs=0, mask=0, flags=0)
    bad = [dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")), dict(scale=float("inf")),
           dict(l2_reg=-0.5), dict(l2_reg=float("nan")), dict(l2_reg=float("inf")), dict(l2_reg=0.5, flags=_ffi.ORX_NO_L2),
           dict(flags=_ffi.ORX_HOGWILD), dict(flags=_ffi.ORX_CENSOR), dict(ci=-64), dict(ci=32), dict(ci=100), dict(cs=-64), dict(cs=32),
           dict(mask=16), dict(mask=_ffi.ORX_TRAIN_BIAS, b=None),
           dict(U=rt.Table(30, 32)), dict(U=rt.Table(30, 260), V=rt.Table(40, 260)), dict(b=rt.Table(40, 2)), dict(b=rt.Table(39, 1)),
           dict(U=rt.Table(30, 64, other)), dict(b=rt.Table(40, 1, other)), dict(opt=_dev_opt(rt, "sgd", other))]
    for kw in bad:
        a = {**base, **kw}
        with pytest.raises(ValueError):
            _raw_step(ctx, a["opt"], a["U"], a["V"], a["b"], uid, pid, a["scale"], a["l2_reg"], a["ci"], a["cs"], a["mask"], a["flags"])
    os.environ["ORX_ADAM_DENSE"] = "1"          # what orx_apply_rows refuses: the whole-table-sweep form of Adam with a bias column
    try:
        with pytest.raises(ValueError, match="ORX_ADAM_DENSE"):
            _raw_step(ctx, _dev_opt(rt, "adam"), *tabs, uid, pid)
    finally:
        del os.environ["ORX_ADAM_DENSE"]
    ctx.synchronize()
    assert _same(before, _bits(*tabs))
    _ffi.check(ctx._lib.orx_fullsoftmax_step(ctx._h, sgd._h, tabs[0]._h, tabs[1]._h, tabs[2]._h, None, None, None, None,
                                             0, 1.0, 0.0, 0, 0, 0, 0, None, None))          # B == 0: ORX_OK, nothing launched
    assert _same(before, _bits(*tabs))
    with pytest.raises(ValueError):
        rt.fullsoftmax_loss(*tabs, uid, pid, scale=0.0)
    with pytest.raises(ValueError):
        rt.SeqRec(tabs[1], rt.Table(40, 64), None).step_full(sgd, (np.arange(66, dtype=np.int32), pid), pid, scale=-1.0)
    from openrec_amd.tf2.recommenders import UCML
    with pytest.raises(NotImplementedError, match="dot products"):
        UCML(8, 8, 10, 10).train_steps_full(sgd, uid, pid)


# ---- 12. the tf2 layer ----------------------------------------------------------------------------------------------------------------
def test_bpr_train_steps_full_is_the_runtime_call():
    rt = _rt()
    from openrec_amd.tf2.recommenders import BPR
    rng = np.random.default_rng(14)
    case = dict(SMALL, bias=False)
    U, V, _, uid, pid = fc.make(case)
    w = _weights(rng, 65); off = _offsets(rng, 40)
    model = BPR(64, 64, case["NU"], case["NI"], use_item_bias=False, l2_reg=0.01)
    model.user_latent_factor.table.write(U); model.item_latent_factor.table.write(V)
    got = model.train_steps_full(_dev_opt(rt, "adagrad"), uid, pid, sample_weight=w, item_offset=off, scale=2.0)
    tabs = _tables(rt, U, V, None)
    want = rt.fullsoftmax_step(_dev_opt(rt, "adagrad"), *tabs, uid, pid, weights=w, item_offset=off, scale=2.0, l2_reg=0.01)
    assert _same_losses(got, want)
    assert _same(_bits(model.user_latent_factor.table, model.item_latent_factor.table), _bits(*tabs))


def test_vanilla_youtube_rec_train_steps_full_is_the_runtime_call():
    rt = _rt()
    from openrec_amd.tf2.recommenders import VanillaYouTubeRec
    case = dict(MID, D=32)
    H, V, b, pid = _seq_tables(rt, case)
    ptr, items = fc.make_bags(case)
    lens = np.diff(ptr)
    L = 6
    seq = np.zeros((case["B"], L), np.int32)
    for i, n in enumerate(lens):
        seq[i, :n] = items[ptr[i]:ptr[i + 1]]
    off = _offsets(np.random.default_rng(1), case["NI"])
    model = VanillaYouTubeRec(32, L, case["NI"], l2_reg_embed=0.01)
    model.seq_item_latent_factor.table.write(H); model.item_latent_factor.table.write(V); model.item_bias.table.write(b)
    fwd = model.loss_full(seq, lens, pid, item_offset=off)
    got = model.train_steps_full(_dev_opt(rt, "adam"), seq, lens, pid, item_offset=off)
    tabs = _tables(rt, H, V, b)
    net = rt.SeqRec(*tabs, pool=("fixed", L))
    want = net.step_full(_dev_opt(rt, "adam"), (ptr, items), pid, item_offset=off, l2_reg=0.01)
    assert _same_losses(got, want) and np.float32(fwd[0]).view(np.int32) == got[0].view(np.int32)[0]
    assert _same(_bits(model.seq_item_latent_factor.table, model.item_latent_factor.table, model.item_bias.table), _bits(*tabs))
