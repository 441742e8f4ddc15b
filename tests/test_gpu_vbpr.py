"""GPU: VBPR (`rt.features_project`, `rt.VBPR`, `openrec_amd.tf2.recommenders.VBPR`) against tests/vbpr_ref.py in float64.  The
cases are tests/vbpr_cases.py's; the two worst-case bounds are vbpr_ref's, whose headroom tests/test_vbpr_cpu.py shows.  Tolerances
are the project's: conftest.delta_check on tables, TOL on loss and l2, TOL_ADAM on Adam's tables.  Where the data is made of small
integers and powers of two every partial sum is representable, and the device must give the float64 result bit for bit."""
import ctypes

import numpy as np
import pytest

import scorer_ref as sr
import vbpr_cases as vc
import vbpr_ref as vr
from conftest import TOL, TOL_ADAM, delta_check, rel_err

pytestmark = pytest.mark.gpu

NAMES = ("U", "V", "b", "E")
ROLE = dict(U="user", V="item", b="bias", E="proj")


def _rt():
    from openrec_amd import runtime as rt
    return rt


def _dev_opt(rt, name):
    lr = vc.LR[name]
    if name == "sgd":
        return rt.Optimizer.sgd(lr)
    if name == "adagrad":
        return rt.Optimizer.adagrad(lr)
    if name == "adam":
        return rt.Optimizer.adam(lr)
    return rt.Optimizer.momentum(lr, 0.9, True)


def _table(rt, a):
    return None if a is None else rt.Table(*a.shape).write(a)


def _net(rt, c):
    """fresh device tables of a case -> (rt.VBPR, {name: table})"""
    t = {k: _table(rt, c[k]) for k in NAMES}
    return rt.VBPR(t["U"], t["V"], t["b"], t["E"], rt.ItemFeatures(c["F"])), t


def _dev(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() if x is not None else None for x in arrays)


def _bits(t):
    return {k: v.read().view(np.int32) for k, v in t.items() if v is not None}


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def _f64(x):
    return None if x is None else x.astype(np.float64)


def _inside(got, want, bound, what):
    err = np.abs(np.asarray(got, np.float64) - want)
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"{what}: worst error {ratio:.3g} of the bound")
    assert np.isfinite(got).all() and (err <= bound).all(), (what, ratio)


# ---- the projection, exact --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (77, 192))
@pytest.mark.parametrize("Fd,Dc", ((1, 1), (50, 20), (64, 32), (200, 128), (515, 33)))
def test_projection_is_exact_on_integer_data(Fd, Dc, n):
    """F integers in [-4, 4], E integers in [-8, 8] times 2^-6: the result equals float64 bit for bit; ids alone, ids and minus (on
    the device), and a row range; into columns [3, 3 + Dc) of a wider table whose other columns and rows stay as they were"""
    rt = _rt()
    NI, col0, SENT = 200, 3, np.float32(7.25)
    rng = np.random.default_rng([Fd, Dc, n])
    F, E = vc.integer_features(rng, NI, Fd, Dc)
    feats, tE = rt.ItemFeatures(F), _table(rt, E)
    assert (feats.rows, feats.dim) == (NI, Fd)
    ia = rng.integers(0, NI, n).astype(np.int32); ib = rng.integers(0, NI, n).astype(np.int32)
    ia[0], ib[0], ib[1] = NI - 1, 0, ia[1]                    # the last row, the first, and a pair that cancels
    dia, dib = _dev(ia, ib)
    for what, kw, want in (("ids", dict(ids=ia), vr.project(F, E, ia)), ("ids - minus", dict(ids=dia, minus=dib), vr.project(F, E, ia, ib)),
                           ("rows", dict(rows=(5, n)), vr.project(F, E, np.arange(5, 5 + n)))):
        out = rt.Table(n + 2, Dc + 5).fill(float(SENT))
        assert rt.features_project(feats, tE, out, col0=col0, **kw) is out
        got = out.read()
        assert np.array_equal(got[:n, col0:col0 + Dc].astype(np.float64), want), (what, Fd, Dc, n)
        rest = np.ones(got.shape, bool); rest[:n, col0:col0 + Dc] = False
        assert (got[rest] == SENT).all(), (what, "columns or rows outside the output were written")


def test_projection_on_float_data_is_inside_the_bound():
    rt = _rt()
    c = vc.make(dict(vc.GENERAL, Fd=515, Dc=33, seed=21))
    feats, tE = rt.ItemFeatures(c["F"]), _table(rt, c["E"])
    ia, ib = c["pid"][0], c["nid"][0]
    out = rt.Table(len(ia), 33)
    got = rt.features_project(feats, tE, out, ids=ia, minus=ib).read()
    _inside(got, vr.project(c["F"], c["E"], ia, ib), vr.proj_bound(c["F"], c["E"], ia, ib), "projection")


# ---- the item table ---------------------------------------------------------------------------------------------------------------
def _item_table_raw(net, W, row0, n):
    from openrec_amd._ffi import check
    f = net.features
    check(net.ctx._lib.orx_vbpr_item_table(net.ctx._h, net.V._h, net.E._h, f.device_ptr, f.rows, f.dim, row0, n, W._h))


@pytest.mark.parametrize("exact", (True, False))
def test_item_table(exact):
    rt = _rt()
    c = vc.make(dict(vc.GENERAL, seed=22))
    if exact:
        c["F"], c["E"] = vc.integer_features(np.random.default_rng(23), c["V"].shape[0], 50, 20)
    net, t = _net(rt, c)
    NI, Dl = c["V"].shape
    W = net.item_table()
    assert W.shape == (NI, Dl + 20) and net.item_table() is W
    got = W.read()
    assert np.array_equal(got[:, :Dl].view(np.int32), c["V"].view(np.int32))
    if exact:
        assert np.array_equal(got[:, Dl:].astype(np.float64), vr.theta(c["F"], c["E"]))
    else:
        _inside(got[:, Dl:], vr.theta(c["F"], c["E"]), vr.proj_bound(c["F"], c["E"], np.arange(NI)), "item table")
    # one call = three calls over row ranges cut at 1 and 7, bit for bit; rows outside a range are not written
    W3 = rt.Table(NI, Dl + 20).fill(-3.5)
    _item_table_raw(net, W3, 1, 6)
    part = W3.read()
    assert (part[:1] == -3.5).all() and (part[7:] == -3.5).all() and np.array_equal(part[1:7].view(np.int32), got[1:7].view(np.int32))
    _item_table_raw(net, W3, 0, 1); _item_table_raw(net, W3, 7, NI - 7)
    assert np.array_equal(W3.read().view(np.int32), got.view(np.int32))
    # rows=(row0, n) refreshes those rows alone
    V2 = (c["V"] * np.float32(2)).astype(np.float32)
    t["V"].write(V2)
    again = net.item_table(rows=(3, 5)).read()
    assert np.array_equal(again[3:8, :Dl], V2[3:8]) and np.array_equal(again[:3], got[:3]) and np.array_equal(again[8:], got[8:])
    net.invalidate()
    assert np.array_equal(net.item_table().read()[:, :Dl], V2)


# ---- the projection gradient ------------------------------------------------------------------------------------------------------
def _dE_through_sgd(rt, c, w, batch_chunk):
    """dE of one batch, read back through an SGD step of lr 1 on a zero-initialised E that trains the projection alone"""
    net, t = _net(rt, dict(c, E=np.zeros_like(c["E"])))
    net.step(rt.Optimizer.sgd(1.0), c["uid"][0], c["pid"][0], c["nid"][0], weights=w, train=("proj",), batch_chunk=batch_chunk)
    return -t["E"].read()


def test_projection_gradient_is_exact_on_representable_data():
    """integer F, U_l = V = 0 and no bias (x = 0: sigmoid = 1/2), weights of 1.5 at B = 192 (w / B = 2^-7), integer U_c: R = g U_c and
    every partial sum of df^T R are representable -- three chunks of 64 give float64's dE bit for bit"""
    rt = _rt()
    c = vc.make(dict(vc.GENERAL, bias=False, seed=24))
    rng = np.random.default_rng(25)
    c["F"], _ = vc.integer_features(rng, c["V"].shape[0], 50, 20)
    c["V"][:] = 0; c["U"][:, :12] = 0
    c["U"][:, 12:] = rng.integers(-3, 4, (c["U"].shape[0], 20))
    w = np.full(192, 1.5, np.float32)
    coef = w[0] * (np.float32(1) / np.float32(192))
    assert coef == np.float32(2.0 ** -7)                      # (what the device forms: w * (1 / B) in fp32)
    ref = vr.grads(_f64(c["U"]), _f64(c["V"]), None, np.zeros((50, 20)), c["F"], c["uid"][0], c["pid"][0], c["nid"][0], _f64(w))
    assert np.array_equal(ref["dE"].astype(np.float32).astype(np.float64), ref["dE"]) and np.abs(ref["dE"]).max() > 0
    got = _dE_through_sgd(rt, c, w, 64)
    assert np.array_equal(got.astype(np.float64), ref["dE"])


@pytest.mark.parametrize("batch_chunk", (64, 0, 128))
def test_projection_gradient_is_inside_the_bound_and_repeatable(batch_chunk):
    rt = _rt()
    c = vc.make(dict(vc.GENERAL, seed=26))
    geo = rt.vbpr_geometry(192, 50, 20, batch_chunk)
    assert geo["chunks"] == {64: 3, 0: 1, 128: 2}[batch_chunk]
    ref = vr.grads(_f64(c["U"]), _f64(c["V"]), _f64(c["b"]), np.zeros((50, 20)), c["F"], c["uid"][0], c["pid"][0], c["nid"][0])
    got = _dE_through_sgd(rt, c, None, batch_chunk)
    _inside(got, ref["dE"], vr.dproj_bound(ref["df"], ref["R"], geo["chunk_rows"], geo["chunks"]), f"dE, batch_chunk {batch_chunk}")
    assert np.abs(got).max() > 0
    assert np.array_equal(_dE_through_sgd(rt, c, None, batch_chunk).view(np.int32), got.view(np.int32))


# ---- the step ---------------------------------------------------------------------------------------------------------------------
def _expect(case, c, l2_reg, l2_proj, train=None):
    t = {k: _f64(c[k]) for k in NAMES}
    oo = vr.make_opt(case["opt"])
    out = [vr.step(t["U"], t["V"], t["b"], t["E"], c["F"], c["uid"][s], c["pid"][s], c["nid"][s], oo,
                   w=None if c["w"] is None else _f64(c["w"][s]), l2_reg=l2_reg, l2_proj=l2_proj, train=train) for s in range(len(c["uid"]))]
    return t, out


def _check(what, case, c, t, want, losses, want_losses, steps):
    for k in NAMES:
        if t[k] is None:
            continue
        got, w32 = t[k].read(), want[k].astype(np.float32)
        print(f"{what} {k}: rel err {rel_err(got, w32):.3g}")
        assert np.isfinite(got).all(), (what, k)
        if case["opt"] == "adam":
            assert rel_err(got, w32) <= TOL_ADAM, (what, k)
        else:
            delta_check(c[k], got, w32, steps=steps, what=f"{what} {k}")
    for s, (lw, l2w) in enumerate(want_losses):
        print(f"{what} step {s}: loss {losses[0][s]:.8g} want {lw:.8g}  l2 {losses[1][s]:.8g} want {l2w:.8g}")
        assert abs(losses[0][s] - lw) <= TOL * abs(lw) and abs(losses[1][s] - l2w) <= TOL * abs(l2w), (what, s)


@pytest.mark.parametrize("case", vc.STEP_CASES, ids=[c["name"] for c in vc.STEP_CASES])
def test_step_matches_the_float64_reference(case):
    rt = _rt()
    c = vc.make(case)
    net, t = _net(rt, c)
    opt = _dev_opt(rt, case["opt"])
    losses = net.step(opt, c["uid"], c["pid"], c["nid"], weights=c["w"], l2_reg=vc.L2_REG, l2_proj=vc.L2_PROJ, K=case["K"])
    want, want_losses = _expect(case, c, vc.L2_REG, vc.L2_PROJ)
    _check(case["name"], case, c, t, want, losses, want_losses, case["K"])
    if case["opt"] == "adam":
        assert opt.step == case["K"]
    # the forward alone, on the tables as they now are
    fl = net.loss(c["uid"][0], c["pid"][0], c["nid"][0], weights=None if c["w"] is None else c["w"][0])
    now = {k: (None if t[k] is None else _f64(t[k].read())) for k in NAMES}
    g = vr.grads(now["U"], now["V"], now["b"], now["E"], c["F"], c["uid"][0], c["pid"][0], c["nid"][0], None if c["w"] is None else _f64(c["w"][0]))
    assert abs(fl[0] - g["loss"]) <= TOL * abs(g["loss"]) and abs(fl[1] - g["l2"]) <= TOL * abs(g["l2"])


@pytest.mark.parametrize("opt", vc.OPTS)
def test_k_steps_are_k_one_step_calls_and_host_ids_are_device_ids(opt):
    rt = _rt()
    case = dict(vc.GENERAL, opt=opt, bias=True, weights=True, K=3, seed=27)
    c = vc.make(case)
    kw = dict(l2_reg=vc.L2_REG, l2_proj=vc.L2_PROJ)
    net, t = _net(rt, c)
    l3 = net.step(_dev_opt(rt, opt), c["uid"], c["pid"], c["nid"], weights=c["w"], K=3, **kw)
    one = _bits(t)
    net, t = _net(rt, c)
    o = _dev_opt(rt, opt)
    l1 = [net.step(o, c["uid"][s], c["pid"][s], c["nid"][s], weights=c["w"][s], **kw) for s in range(3)]
    assert _same(one, _bits(t)), "a K = 3 call differs from three one-step calls"
    assert all(np.array_equal(l3[j][s:s + 1].view(np.int32), l1[s][j].view(np.int32)) for s in range(3) for j in range(2))
    net, t = _net(rt, c)
    du, dp, dn, dw = _dev(c["uid"], c["pid"], c["nid"], c["w"])
    ld = net.step(_dev_opt(rt, opt), du, dp, dn, weights=dw, K=3, **kw)
    assert _same(one, _bits(t)), "device ids give other bits than host ids"
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(l3, ld))
    net, t = _net(rt, c)
    assert net.step(_dev_opt(rt, opt), du, dp, dn, weights=dw, K=3, want_loss=False, **kw) is None
    assert _same(one, _bits(t))


def test_identity_features_make_it_bpr_on_the_concatenated_item_table():
    """F = I (NI = Fd = 64), l2_reg = l2_proj = 0: the model is BPR on the item table [V | E] -- a check that never sees the projection"""
    rt = _rt()
    NU, NI, Dl, Dc, B = 200, 64, 12, 20, 96
    rng = np.random.default_rng(28)
    c = vc.make(dict(NU=NU, NI=NI, Fd=NI, Dl=Dl, Dc=Dc, B=B, seed=29))
    c["F"] = np.eye(NI, dtype=np.float32)
    items = rng.permutation(np.tile(np.arange(NI, dtype=np.int32), 3))          # every item three times over the 2B lookups
    uid, pid, nid = c["uid"][0], items[:B].copy(), items[B:].copy()
    assert np.bincount(np.concatenate([pid, nid])).max() <= 4
    net, t = _net(rt, c)
    net.step(rt.Optimizer.sgd(0.05), uid, pid, nid)
    VE = np.concatenate([c["V"], c["E"]], 1)
    tU, tVE, tb = _table(rt, c["U"]), _table(rt, VE), _table(rt, c["b"])
    rt.pairwise_step("bpr", rt.Optimizer.sgd(0.05), tU, tVE, tb, uid, pid, nid, no_l2=True)
    want = tVE.read()
    assert np.abs(want - VE).max() > 0
    delta_check(c["U"], t["U"].read(), tU.read(), what="user")
    delta_check(c["V"], t["V"].read(), np.ascontiguousarray(want[:, :Dl]), what="item")
    delta_check(c["E"], t["E"].read(), np.ascontiguousarray(want[:, Dl:]), what="proj")
    delta_check(c["b"], t["b"].read(), tb.read(), what="bias")


# ---- the train mask ---------------------------------------------------------------------------------------------------------------
def _slots(rt, opt, t):
    return {f"{k}{s}": opt.slot(v, s).view(np.int32) for k, v in t.items() if v is not None for s in range(rt.Optimizer.NSLOTS[opt.kind])}


def _two_steps(rt, c, optname, train):
    """a full step, then a step with `train` -> (tables, slots and counter after step 1, after step 2)"""
    net, t = _net(rt, c)
    opt = _dev_opt(rt, optname)
    kw = dict(l2_reg=vc.L2_REG, l2_proj=vc.L2_PROJ)
    net.step(opt, c["uid"][0], c["pid"][0], c["nid"][0], **kw)
    first = (_bits(t), _slots(rt, opt, t), opt.step)
    net.step(opt, c["uid"][1], c["pid"][1], c["nid"][1], train=train, **kw)
    return first, (_bits(t), _slots(rt, opt, t), opt.step)


@pytest.mark.parametrize("optname", ("sgd", "adam"))
def test_train_mask(optname):
    rt = _rt()
    c = vc.make(dict(vc.GENERAL, bias=True, K=2, seed=30))
    _, full = _two_steps(rt, c, optname, None)
    for train in (("user",), ("item",), ("bias",), ("proj",), ("user", "proj")):
        first, second = _two_steps(rt, c, optname, train)
        for k in NAMES:
            inside = ROLE[k] in train
            ref = full if inside else first
            assert np.array_equal(second[0][k], ref[0][k]), (optname, train, k, "inside" if inside else "outside")
            for s in range(rt.Optimizer.NSLOTS[optname]):
                assert np.array_equal(second[1][f"{k}{s}"], ref[1][f"{k}{s}"]), (optname, train, k, "slot", s)
            assert not inside or not np.array_equal(second[0][k], first[0][k])
        if optname == "adam":
            assert (first[2], second[2]) == (1, 2)


# ---- serving ----------------------------------------------------------------------------------------------------------------------
def test_serving_paths_take_the_item_table():
    rt = _rt()
    c = vc.make(dict(vc.GENERAL, seed=31))
    NI, Dl = c["V"].shape
    c["F"], c["E"] = vc.integer_features(np.random.default_rng(32), NI, 50, 20)        # theta is exact: one rounding, none at all
    net, t = _net(rt, c)
    Wref = np.concatenate([c["V"], vr.theta(c["F"], c["E"]).astype(np.float32)], 1)
    tW = _table(rt, Wref)
    uid = np.array([0, 7, 299, 7], np.int32)
    rng = np.random.default_rng(33)
    draws = [rng.choice(NI, 14, replace=False) for _ in uid]
    pos = rt.SparseMask.from_lists([d[:5] for d in draws], NI)
    excl = rt.SparseMask.from_lists([d[5:] for d in draws], NI)
    cand = [rng.integers(0, NI, 13) for _ in uid]
    first = None
    for item in (net.item_table(), tW):
        out = (rt.recommend_topk("dot", t["U"], item, t["b"], uid, 10, excl=excl), rt.rank_metrics_matrixfree(pos, excl, [5, 20], "dot", t["U"], item, t["b"], uid),
               rt.score_candidates("dot", t["U"], item, t["b"], uid, cand), np.asarray(rt.score_all_items("dot", t["U"], item, t["b"], uid)))
        if item is tW:
            assert np.array_equal(out[0][0], first[0][0]) and np.array_equal(out[0][1].view(np.int32), first[0][1].view(np.int32))
            assert all(np.array_equal(out[1][k].view(np.int32), first[1][k].view(np.int32)) for k in ("auc", "ndcg", "recall"))
            assert np.array_equal(out[2].view(np.int32), first[2].view(np.int32))
        first = out
    sr.check(first[3], "dot", c["U"], Wref, c["b"], None, uid, "scores on the item table")        # the scorer's own tolerance
    # a step, then item_table() without invalidate(): the new V and E
    net.step(rt.Optimizer.sgd(0.05), c["uid"][0], c["pid"][0], c["nid"][0], l2_reg=vc.L2_REG)
    got, V1, E1 = net.item_table().read(), t["V"].read(), t["E"].read()
    assert not np.array_equal(V1, c["V"]) and not np.array_equal(E1, c["E"])
    assert np.array_equal(got[:, :Dl].view(np.int32), V1.view(np.int32))
    _inside(got[:, Dl:], vr.theta(c["F"], E1), vr.proj_bound(c["F"], E1, np.arange(NI)), "item table after a step")


# ---- errors -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("uid", "pid", "nid"))
def test_an_id_outside_its_table_raises_and_leaves_the_other_triplets_their_step(which):
    """the bad triplet contributes nothing: the tables get the bits of the same batch with that triplet valid at weight 0 (l2_reg = 0)"""
    rt = _rt()
    c = vc.make(dict(vc.GENERAL, seed=34))
    ids = {k: c[k][0].copy() for k in ("uid", "pid", "nid")}
    good = {k: v.copy() for k, v in ids.items()}
    ids[which][17] = c["U"].shape[0] if which == "uid" else c["V"].shape[0]
    w1, w0 = np.ones(192, np.float32), np.ones(192, np.float32)
    w0[17] = 0
    net, t = _net(rt, c)
    with pytest.raises(IndexError):
        net.step(rt.Optimizer.sgd(0.05), ids["uid"], ids["pid"], ids["nid"], weights=w1, l2_proj=vc.L2_PROJ)
    bad = _bits(t)
    net, t = _net(rt, c)
    net.step(rt.Optimizer.sgd(0.05), good["uid"], good["pid"], good["nid"], weights=w0, l2_proj=vc.L2_PROJ)
    assert _same(bad, _bits(t))
    assert not np.array_equal(bad["U"], c["U"].view(np.int32))
    net.step(rt.Optimizer.sgd(0.05), good["uid"], good["pid"], good["nid"])          # the context stays usable
    with pytest.raises(IndexError):
        rt.features_project(net.features, t["E"], rt.Table(4, 20), ids=np.array([0, 400, 1, 2], np.int32))


def test_bad_arguments_are_refused_before_any_launch():
    rt = _rt()
    from openrec_amd import _ffi
    c = vc.make(dict(vc.GENERAL, seed=35))
    net, t = _net(rt, c)
    before = _bits(t)
    ids = (c["uid"][0], c["pid"][0], c["nid"][0])
    opt = rt.Optimizer.sgd(0.05)
    T = rt.Table
    feats = net.features
    with pytest.raises(ValueError):
        rt.VBPR(T(300, 12), t["V"], t["b"], T(50, 0), feats)                                  # Dc = 0
    with pytest.raises(ValueError, match="above 128"):
        rt.VBPR(T(300, 141), t["V"], t["b"], T(50, 129), feats)
    with pytest.raises(ValueError, match="ItemFeatures"):
        rt.ItemFeatures(np.zeros((400, 0), np.float32))                                        # Fd = 0
    with pytest.raises(ValueError, match="above 256"):
        rt.VBPR(T(300, 257), T(400, 200), None, T(50, 57), feats)
    with pytest.raises(ValueError, match="batch_chunk"):
        net.step(opt, *ids, batch_chunk=96)
    with pytest.raises(ValueError, match="feature rows"):
        rt.VBPR(t["U"], t["V"], t["b"], t["E"], rt.ItemFeatures(c["F"][:399]))
    with pytest.raises(ValueError, match='"bias" named'):
        rt.VBPR(t["U"], t["V"], None, t["E"], feats).step(opt, *ids, train=("bias",))
    # the library itself refuses them too (ORX_ERR_ARG), whatever the Python layer lets through
    lib, h = net.ctx._lib, net.ctx._h
    p = [a.ctypes.data for a in ids]

    def raw(b=t["b"], E=t["E"], Fd=50, NI=400, chunk=0, mask=0, flags=0, l2p=0.0):
        return lib.orx_vbpr_step(h, opt._h, t["U"]._h, t["V"]._h, b._h if b is not None else None, E._h, feats.device_ptr, NI, Fd, *p, None,
                                 1, 192, 192, 0.0, l2p, chunk, mask, flags, None, None)

    for kw in (dict(chunk=96), dict(chunk=-64), dict(mask=_ffi.ORX_TRAIN_BIAS, b=None), dict(mask=16), dict(flags=_ffi.ORX_HOGWILD),
               dict(flags=_ffi.ORX_CENSOR), dict(Fd=0), dict(Fd=49), dict(NI=399), dict(E=T(50, 21)), dict(l2p=-1.0),
               dict(flags=_ffi.ORX_NO_L2, l2p=0.5)):
        assert raw(**kw) == _ffi.ORX_ERR_ARG, kw
    net.ctx.synchronize()
    assert _same(before, _bits(t))


def test_nan_features_reach_exactly_the_outputs_that_depend_on_them():
    rt = _rt()
    c = vc.make(dict(vc.GENERAL, seed=36))
    c["F"][123, 7] = np.nan
    net, t = _net(rt, c)
    W = net.item_table().read()
    assert np.isnan(W[123, 12:]).all() and np.isfinite(np.delete(W, 123, 0)).all() and np.isfinite(W[123, :12]).all()
    ia, ib = c["pid"][0].copy(), c["nid"][0].copy()
    ia[5], ib[9] = 123, 123
    hit = (ia == 123) | (ib == 123)
    got = rt.features_project(net.features, t["E"], rt.Table(192, 20), ids=ia, minus=ib).read()
    assert np.isnan(got[hit]).all() and np.isfinite(got[~hit]).all() and hit.sum() >= 2


# ---- the reference-shaped class ---------------------------------------------------------------------------------------------------
def test_tf2_class_trains_as_the_runtime_and_serves_new_items():
    rt = _rt()
    from openrec_amd.tf2.recommenders import VBPR
    c = vc.make(dict(vc.GENERAL, bias=True, weights=True, K=2, seed=37))
    NU, NI, Dl = 300, 400, 12
    model = VBPR(dim_user_embed=32, dim_item_embed=Dl, total_users=NU, total_items=NI, item_features=c["F"], l2_reg=vc.L2_REG, l2_reg_mlp=vc.L2_PROJ)
    lfs = dict(U=model.user_latent_factor, V=model.item_latent_factor, b=model.item_bias, E=model.projection)
    assert lfs["E"].table.shape == (50, 20) and len(model.trainable_variables) == 4
    c.update({k: lf.table.read() for k, lf in lfs.items()})
    net, t = _net(rt, c)
    got = model.train_steps(rt.Optimizer.adagrad(0.05), c["uid"], c["pid"], c["nid"], sample_weight=c["w"])
    want = net.step(rt.Optimizer.adagrad(0.05), c["uid"], c["pid"], c["nid"], weights=c["w"], l2_reg=vc.L2_REG, l2_proj=vc.L2_PROJ, K=2)
    assert _same({k: lf.table.read().view(np.int32) for k, lf in lfs.items()}, _bits(t))
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got, want))
    assert model.loss(c["uid"][0], c["pid"][0], c["nid"][0]) == net.loss(c["uid"][0], c["pid"][0], c["nid"][0])
    # inference is the scorer on (U, [V | F E], b)
    U, V, b, E = (t[k].read() for k in NAMES)
    uid = np.array([3, 250], np.int32)
    sr.check(np.asarray(model.inference(uid)), "dot", U, np.concatenate([V, vr.theta(c["F"], E).astype(np.float32)], 1), b, None, uid, "inference")
    # a new item's features: aimed at user 3 so that it outranks everything once the row is in place
    j = 77
    ids0, _ = model.recommend(uid[:1], 1)
    d = _f64(E) @ _f64(U[3, Dl:])
    f = (10.0 / float(d @ d) * d).astype(np.float32)
    assert ids0[0, 0] != j
    model.set_item_features([j], f[None, :])
    ids1, sc1 = model.recommend(uid[:1], 1)
    expect = float(_f64(U[3, :Dl]) @ _f64(V[j]) + _f64(U[3, Dl:]) @ (_f64(f) @ _f64(E)) + b[j, 0])
    assert ids1[0, 0] == j and abs(sc1[0, 0] - expect) <= 1e-4 * abs(expect)
    assert np.array_equal(model.item_features.read()[j], f)
