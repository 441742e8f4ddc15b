"""GPU: the history-pooled sequence recommender (`rt.bag_pool`, `rt.SeqRec`, `recommenders.VanillaYouTubeRec`) against
tests/seqrec_ref.py in float64, rounded to float32 once.  The cases are tests/seqrec_cases.py's.  Tolerances are the project's:
conftest.delta_check on tables, TOL on loss and l2, TOL_ADAM on Adam's tables; the pooling itself is held to seqrec_ref.pool_bound
(whose headroom tests/test_seqrec_cpu.py shows) and, on integer data, to equality."""
import numpy as np
import pytest

import multineg_cases as mc
import seqrec_cases as sc
import seqrec_ref as sr
from conftest import TOL, TOL_ADAM, delta_check, rel_err

pytestmark = pytest.mark.gpu

POOLS = ("mean", "sum", sc.FIXED)
BY_NAME = {c["name"]: c for c in sc.CASES}


def _rt():
    from openrec_amd import runtime as rt
    return rt


def _dev_opt(rt, name):
    lr = mc.LR[name]
    if name == "sgd":
        return rt.Optimizer.sgd(lr)
    if name == "adagrad":
        return rt.Optimizer.adagrad(lr)
    if name == "adam":
        return rt.Optimizer.adam(lr)
    return rt.Optimizer.momentum(lr, 0.9, True)


def _tables(rt, *arrays):
    return tuple(rt.Table(*x.shape).write(x) if x is not None else None for x in arrays)


def _dev(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() if x is not None else None for x in arrays)


def _bits(*tables):
    return [t.read().view(np.int32) for t in tables if t is not None]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _f32bits(x):
    return np.asarray(x, np.float32).view(np.int32)


def _padded(ptr, items, rng, garbage=True):
    """the ragged lists as the padded pair (seq [B, L], seq_len [B]) with garbage beyond seq_len"""
    lens = np.diff(ptr)
    L = max(int(lens.max()), 1) + 3
    seq = np.full((len(lens), L), -7, np.int32)
    if garbage:
        seq = rng.choice(np.array([-1, 2 ** 31 - 1, -2 ** 31, 10 ** 6], np.int64), (len(lens), L)).astype(np.int32)
    for i, n in enumerate(lens):
        seq[i, :n] = items[ptr[i]:ptr[i + 1]]
    return seq, lens.astype(np.int32)


def _net(rt, case, tabs):
    return rt.SeqRec(*tabs, pool=case["pool"])


def _step(net, opt, case, bt, device=False, **kw):
    args = (bt["ptr"], bt["items"], bt["pid"], bt["nid"], bt["w"], bt["off"])
    if device:
        args = _dev(*args)
    return net.step(opt, (args[0], args[1]), args[2], args[3], loss=case["kind"], weights=args[4], neg_offset=args[5], **kw)


def _expect(case, H, V, b, batches, l2_reg):
    """the float64 reference -> tables (float64, stepped in place on copies), [(loss, l2)] per step"""
    H, V = H.astype(np.float64), V.astype(np.float64)
    b = b.astype(np.float64) if b is not None else None
    oo = mc.make_opt(case["opt"])
    out = [sr.step(case["kind"], H, V, b, bt["ptr"], bt["items"], bt["pid"], bt["nid"], oo, case["pool"], w=bt["w"], off=bt["off"],
                   l2_reg=l2_reg) for bt in batches]
    return (H, V, b), out


def _check(what, case, orig, tabs, want, losses, want_losses, steps):
    for name, W0, t, w in zip(("history", "item", "bias"), orig, tabs, want):
        if t is None:
            continue
        got, w32 = t.read(), w.astype(np.float32)
        print(f"{what} {name}: rel err {rel_err(got, w32):.3g}")
        assert np.isfinite(got).all(), (what, name)
        if case["opt"] == "adam":
            assert rel_err(got, w32) <= TOL_ADAM, (what, name)
        else:
            delta_check(W0, got, w32, steps=steps, what=f"{what} {name}")
    for s, ((lg, l2g), (lw, l2w)) in enumerate(zip(losses, want_losses)):
        print(f"{what} step {s}: loss {lg:.8g} want {lw:.8g}  l2 {l2g:.8g} want {l2w:.8g}")
        assert abs(lg - lw) <= TOL * abs(lw) and abs(l2g - l2w) <= TOL * abs(l2w), (what, s)


# ---- 1. integer data: exact ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 3, 64, 100, 256])
def test_bag_pool_on_integer_data_is_exact(D):
    """H holds integers in [-8, 8] times 2^-6; sums, and means at power-of-two lengths, equal float64 bit for bit -- with host
    lists, device lists and the padded form with garbage padding; rows of out outside [row0, row0 + B) keep a sentinel"""
    rt = _rt()
    rng = np.random.default_rng(5)
    NI, B, row0 = 200, 70, 5
    H = (rng.integers(-8, 9, (NI, D)) * 2.0 ** -6).astype(np.float32)
    lens = rng.choice(np.array([0, 1, 2, 4, 64, 128]), B)
    lens[:3] = (128, 64, 0)
    ptr = np.zeros(B + 1, np.int32); ptr[1:] = np.cumsum(lens)
    items = rng.integers(0, NI, ptr[-1]).astype(np.int32)
    tH, = _tables(rt, H)
    for pool in ("sum", "mean"):
        want, _ = sr.pool_rows(H.astype(np.float64), ptr, items, pool)
        want = want.astype(np.float32)
        assert np.array_equal(want.astype(np.float64), sr.pool_rows(H.astype(np.float64), ptr, items, pool)[0])      # representable
        for form in ("host", "device", "padded", "padded-device"):
            bags = (ptr, items)
            if form.startswith("padded"):
                bags = _padded(ptr, items, rng)
            if form.endswith("device"):
                bags = _dev(*bags)
            out = rt.Table(B + 9, D).fill(-123.0)
            rt.bag_pool(tH, bags, out, pool=pool, rows=(row0, B))
            tH.ctx.check_index_error()
            got = out.read()
            assert np.array_equal(_f32bits(got[row0:row0 + B]), _f32bits(want)), (pool, form)
            assert (got[:row0] == -123.0).all() and (got[row0 + B:] == -123.0).all(), (pool, form)


# ---- 2. float data: inside the bound ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", POOLS, ids=sc._pool_name)
@pytest.mark.parametrize("D", [1, 3, 64, 100, 256])
def test_bag_pool_on_float_data_is_inside_pool_bound(D, pool):
    rt = _rt()
    rng = np.random.default_rng(6)
    NI, B = 150, 300
    H = rng.uniform(-1, 1, (NI, D)).astype(np.float32)
    ptr, items = sc.make_bags(rng, B, NI)
    tH, = _tables(rt, H)
    out = rt.Table(B, D).fill(7.0)
    rt.bag_pool(tH, (ptr, items), out, pool=pool)
    got = out.read()
    H64 = H.astype(np.float64)
    want, c64 = sr.pool_rows(H64, ptr, items, pool)
    bound = sr.pool_bound(H, ptr, items, c64)
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"D={D} pool={sc._pool_name(pool)}: worst |err| / bound {ratio:.3g}")
    assert (err <= bound).all()
    empty = np.diff(ptr) == 0
    assert empty.any() and np.array_equal(_f32bits(got[empty]), np.zeros((int(empty.sum()), D), np.int32))      # +0, not -0


# ---- 3. the bits of a bag are its own ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [3, 64, 100, 256])
def test_a_bag_pools_to_the_same_bits_alone_in_a_batch_and_at_another_row(D):
    rt = _rt()
    rng = np.random.default_rng(7)
    NI, B = 120, 64
    H = rng.uniform(-1, 1, (NI, D)).astype(np.float32)
    ptr, items = sc.make_bags(rng, B, NI)
    tH, = _tables(rt, H)
    for pool in POOLS:
        whole = rt.bag_pool(tH, (ptr, items), rt.Table(B, D), pool=pool).read()
        shifted = rt.bag_pool(tH, _dev(ptr, items), rt.Table(B + 11, D), pool=pool, rows=(11, B)).read()[11:]
        one = rt.Table(B, D)
        for i in range(B):
            rt.bag_pool(tH, (np.array([0, ptr[i + 1] - ptr[i]], np.int32), items[ptr[i]:ptr[i + 1]]), one, pool=pool, rows=(i, 1))
        assert np.array_equal(_f32bits(whole), _f32bits(shifted)) and np.array_equal(_f32bits(whole), _f32bits(one.read())), pool


# ---- 4. the loss is multineg's on the pooled rows, the step's loss is the forward's -------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in sc.CASES[:6]])
def test_loss_is_multineg_loss_on_the_pooled_table_and_the_steps_own(name):
    rt = _rt()
    case = BY_NAME[name]
    H, V, b = sc.make_tables(case)
    bt = sc.make_batches(case)[0]
    tabs = _tables(rt, H, V, b)
    net = _net(rt, case, tabs)
    bags = (bt["ptr"], bt["items"])
    kw = dict(loss=case["kind"], weights=bt["w"], neg_offset=bt["off"])
    before = _bits(*tabs)
    fwd = net.loss(bags, bt["pid"], bt["nid"], **kw)
    Q = net.user_table(bags)
    ref = rt.multineg_loss(case["kind"], Q, tabs[1], tabs[2], np.arange(case["B"], dtype=np.int32), bt["pid"], bt["nid"],
                           weights=bt["w"], neg_offset=bt["off"])
    assert np.array_equal(_f32bits(fwd), _f32bits(ref))
    dfwd = net.loss(_dev(*bags), *_dev(bt["pid"], bt["nid"]), loss=case["kind"], weights=_dev(bt["w"])[0], neg_offset=_dev(bt["off"])[0])
    assert dfwd == fwd
    assert _same(before, _bits(*tabs))
    loss, l2 = net.step(_dev_opt(rt, case["opt"]), bags, bt["pid"], bt["nid"], l2_reg=0.01, **kw)
    assert np.array_equal(_f32bits([loss[0], l2[0]]), _f32bits(fwd))


# ---- 5. the item apply is multineg's, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("D", [64, 100, 3])
def test_item_table_after_a_step_is_the_one_multineg_step_leaves(opt, D):
    rt = _rt()
    case = dict(sc.CASES[0], D=D, opt=opt, bias=False, seed=31)
    H, V, _ = sc.make_tables(case)
    bt = sc.make_batches(case)[0]
    tH, tV = _tables(rt, H, V)
    net = rt.SeqRec(tH, tV, None, pool="mean")
    bags = (bt["ptr"], bt["items"])
    Q = rt.Table(case["B"], D)
    net.user_table(bags, out=Q)
    tV2, = _tables(rt, V)
    for l2_reg in (0.0, 0.05):
        net.step(_dev_opt(rt, opt), bags, bt["pid"], bt["nid"], loss=case["kind"], l2_reg=l2_reg, train=None)
        rt.multineg_step(case["kind"], _dev_opt(rt, opt), Q, tV2, None, np.arange(case["B"], dtype=np.int32), bt["pid"], bt["nid"],
                         l2_reg=l2_reg)
        assert _same(_bits(tV), _bits(tV2)), l2_reg
        net.user_table(bags, out=Q)              # (the next round starts from the same state on both sides: H moved, so did Q)


# ---- 6. the tables against the float64 reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.CASES, ids=[c["name"] for c in sc.CASES])
def test_step_matches_the_float64_reference(case):
    rt = _rt()
    H, V, b = sc.make_tables(case)
    batches = sc.make_batches(case)
    l2_reg = 0.01 if case["seed"] % 2 else 0.0
    tabs = _tables(rt, H, V, b)
    net = _net(rt, case, tabs)
    opt = _dev_opt(rt, case["opt"])
    losses = []
    want, want_losses = _expect(case, H, V, b, batches, l2_reg)
    first, _ = _expect(case, H, V, b, batches[:1], l2_reg)
    for s, bt in enumerate(batches):
        loss, l2 = _step(net, opt, case, bt, device=bool(s % 2), l2_reg=l2_reg)
        losses.append((loss[0], l2[0]))
        if s == 0:
            _check(case["name"] + " after one step", case, (H, V, b), tabs, first, losses, want_losses, 1)
    if len(batches) > 1:
        _check(case["name"], case, (H, V, b), tabs, want, losses, want_losses, len(batches))


# ---- 7. repeatable bits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", mc.OPTS)
def test_two_runs_from_the_same_state_give_the_same_bits(opt):
    rt = _rt()
    case = dict(sc.CASES[9], opt=opt, bias=False)
    H, V, _ = sc.make_tables(case)
    batches = sc.make_batches(case)
    runs = []
    for r in range(2):
        tabs = _tables(rt, H, V, None)
        net = _net(rt, case, tabs)
        o = _dev_opt(rt, opt)
        ls = [_step(net, o, case, bt, device=bool(r), l2_reg=0.01) for bt in batches]
        runs.append((_bits(*tabs), np.concatenate([_f32bits(x) for l in ls for x in l])))
    assert _same(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])      # (host lists and device lists: the same bits)


# ---- 8. train masks --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["sgd", "adagrad", "adam", "momentum"])
@pytest.mark.parametrize("train", [("history",), ("item",), ("item", "bias")])
def test_train_masks_freeze_tables_and_slots(opt, train):
    """the frozen tables and their optimizer slots keep their bits.  The trained ones equal the full step's: bit for bit where
    both take the sorted apply (the history table always; the item table without a bias), inside the update bound where the
    full step applies item and bias together (that apply adds with atomics, as orx_multineg_step's)"""
    rt = _rt()
    case = dict(sc.CASES[0], opt=opt, bias=True, NI=300, N=1, seed=41)      # (few occurrences per item row: see seqrec_cases on SGD with a bias)
    H, V, b = sc.make_tables(case)
    batches = sc.make_batches(dict(case, steps=2))
    names = ("history", "item", "bias")

    def run(train):
        tabs = _tables(rt, H, V, b)
        net = _net(rt, case, tabs)
        o = _dev_opt(rt, opt)
        slots0 = None
        for s, bt in enumerate(batches):
            if s == 1:
                slots0 = [[o.slot(t, k) for k in range(rt.Optimizer.NSLOTS[opt])] for t in tabs]
                before = [t.read() for t in tabs]
            _step(net, o, case, bt, l2_reg=0.01, train=train if s == 1 else None)
        slots1 = [[o.slot(t, k) for k in range(rt.Optimizer.NSLOTS[opt])] for t in tabs]
        return [t.read() for t in tabs], before, slots0, slots1

    full, before, _, _ = run(None)
    got, before_m, s0, s1 = run(train)
    for i, name in enumerate(names):
        if name in train:
            if name == "history":
                assert np.array_equal(_f32bits(got[i]), _f32bits(full[i])), name
            elif opt == "adam":
                assert rel_err(got[i], full[i]) <= TOL_ADAM, name
            else:
                delta_check(before[i], got[i], full[i], steps=1, what=f"{opt} {train} {name}")
            assert not np.array_equal(got[i], before_m[i]), name
        else:
            assert np.array_equal(_f32bits(got[i]), _f32bits(before_m[i])), name
            for a, c in zip(s0[i], s1[i]):
                assert np.array_equal(_f32bits(a), _f32bits(c)), name


# ---- 9. errors -------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable():
    rt = _rt()
    case = sc.CASES[0]
    H, V, b = sc.make_tables(case)
    bt = sc.make_batches(case)[0]
    ptr, items, NI = bt["ptr"], bt["items"], case["NI"]
    tabs = _tables(rt, H, V, b)
    net = _net(rt, case, tabs)
    opt = _dev_opt(rt, "sgd")

    def valid_step_matches():
        for t, x in zip(tabs, (H, V, b)):
            if t is not None:
                t.write(x)
        loss, l2 = _step(net, opt, case, bt, l2_reg=0.01)
        want, wl = _expect(dict(case, opt="sgd"), H, V, b, [bt], 0.01)
        _check("after an error", dict(case, opt="sgd"), (H, V, b), tabs, want, [(loss[0], l2[0])], wl, 1)

    dec = ptr.copy(); dec[5] = dec[4] - 1
    short = ptr.copy(); short[-1] -= 1
    for bad in (dec, short):
        with pytest.raises(ValueError):
            net.step(opt, (bad, items), bt["pid"], bt["nid"])
        with pytest.raises(ValueError):
            rt.bag_pool(tabs[0], (bad, items), rt.Table(case["B"], case["D"]))
        with pytest.raises(IndexError):
            net.step(opt, _dev(bad, items), *_dev(bt["pid"], bt["nid"]))
        valid_step_matches()
    for bad_id in (NI, -1):
        it = items.copy(); it[ptr[3] + 1] = bad_id
        with pytest.raises(IndexError):
            net.step(opt, (ptr, it), bt["pid"], bt["nid"])
        valid_step_matches()
        with pytest.raises(IndexError):
            rt.bag_pool(tabs[0], (ptr, it), rt.Table(case["B"], case["D"]))
        assert all(np.isfinite(t.read()).all() for t in tabs if t is not None)
    with pytest.raises(ValueError):
        rt.SeqRec(tabs[0], tabs[0], None)
    with pytest.raises(ValueError):
        rt.SeqRec(rt.Table(NI, 257), rt.Table(NI, 257), None)
    # the library's own refusals, past the Python layer
    from openrec_amd import _ffi
    ctx = tabs[0].ctx
    t257 = rt.Table(NI, 257), rt.Table(NI, 257)
    pid, nid = bt["pid"], bt["nid"]

    def raw(hist, item, p=ptr, flags=0, mode=0, denom=1.0, N=case["N"], l2=0.0):
        return ctx._lib.orx_seqrec_step(ctx._h, 0, opt._h, hist._h, item._h, None, p.ctypes.data, items.ctypes.data, pid.ctypes.data,
                                        nid.ctypes.data, None, None, case["B"], len(items), N, mode, denom, l2, 0, flags, None, None)

    before = _bits(*tabs)
    assert raw(tabs[0], tabs[0]) == _ffi.ORX_ERR_ARG and raw(*t257) == _ffi.ORX_ERR_ARG
    assert raw(tabs[0], tabs[1], p=dec) == _ffi.ORX_ERR_ARG and raw(tabs[0], tabs[1], p=short) == _ffi.ORX_ERR_ARG
    assert raw(tabs[0], tabs[1], mode=2) == _ffi.ORX_ERR_ARG and raw(tabs[0], tabs[1], mode=1, denom=0.0) == _ffi.ORX_ERR_ARG
    assert raw(tabs[0], tabs[1], N=65) == _ffi.ORX_ERR_ARG and raw(tabs[0], tabs[1], l2=-1.0) == _ffi.ORX_ERR_ARG
    assert raw(tabs[0], tabs[1], flags=_ffi.ORX_HOGWILD) == _ffi.ORX_ERR_ARG and raw(tabs[0], tabs[1], flags=_ffi.ORX_CENSOR) == _ffi.ORX_ERR_ARG
    assert _same(before, _bits(*tabs))


# ---- 10. serving ------------------------------------------------------------------------------------------------------------------------
def test_recommend_is_topk_on_the_pooled_table_and_the_tf2_class_agrees():
    rt = _rt()
    from openrec_amd.tf2.recommenders import VanillaYouTubeRec
    case = dict(sc.CASES[0], NI=300, bias=True, seed=51)
    H, V, b = sc.make_tables(case)
    bt = sc.make_batches(case)[0]
    rng = np.random.default_rng(52)
    tabs = _tables(rt, H, V, b)
    net = rt.SeqRec(*tabs, pool=case["pool"])
    bags = (bt["ptr"], bt["items"])
    B = case["B"]
    excl = rt.SparseMask.from_lists([np.unique(bt["items"][bt["ptr"][i]:bt["ptr"][i + 1]]) for i in range(B)], case["NI"])
    got = net.recommend(bags, 20, excl)
    want = rt.recommend_topk("dot", net.user_table(bags), tabs[1], tabs[2], np.arange(B, dtype=np.int32), 20, excl)
    assert np.array_equal(got[0], want[0]) and np.array_equal(_f32bits(got[1]), _f32bits(want[1]))
    scores = net.user_table(bags).read().astype(np.float64) @ V.astype(np.float64).T + b.astype(np.float64)[:, 0]
    top = np.take_along_axis(scores, got[0].astype(np.int64), 1)
    assert np.abs(top - got[1]).max() <= 1e-5 * np.abs(scores).max()
    # the tf2 class on the same tables: padded inputs, pool = ("fixed", L)
    seq, seq_len = _padded(bt["ptr"], bt["items"], rng)
    L = seq.shape[1]
    # (without the bias table: the item table then takes the sorted apply and both sides have the same bits)
    model = VanillaYouTubeRec(dim_item_embed=case["D"], max_seq_len=L, total_items=case["NI"], l2_reg_embed=0.01, use_item_bias=False)
    for lf, x in zip((model.seq_item_latent_factor, model.item_latent_factor), (H, V)):
        lf.table.write(x)
    net2 = rt.SeqRec(*_tables(rt, H, V), pool=("fixed", L))
    o1, o2 = _dev_opt(rt, "adagrad"), _dev_opt(rt, "adagrad")
    l1 = model.train_steps(o1, seq, seq_len, bt["pid"], bt["nid"], loss="softmax")
    l2 = net2.step(o2, bags, bt["pid"], bt["nid"], loss="softmax", l2_reg=0.01)
    assert np.array_equal(_f32bits(l1), _f32bits(l2))
    assert _same(_bits(model.seq_item_latent_factor.table, model.item_latent_factor.table), _bits(net2.H, net2.V))
    inf = np.asarray(model.inference(seq, seq_len))
    ref = rt.score_all_items("dot", net2.user_table(bags), net2.V, net2.b, np.arange(B, dtype=np.int32))
    assert inf.shape == (B, case["NI"]) and np.array_equal(_f32bits(inf), _f32bits(ref))
    r1 = model.recommend(seq, seq_len, 10)
    r2 = net2.recommend(bags, 10)
    assert np.array_equal(r1[0], r2[0])
    cand = [np.array([1, 5, 9, 5], np.int32) + i % 3 for i in range(B)]
    for i, row in enumerate(model.score(seq, seq_len, cand)):
        assert np.array_equal(_f32bits(row), _f32bits(ref[i, cand[i]])), i
    uid = np.arange(B, dtype=np.int32)
    pos = rt.SparseMask.from_lists([[int(x)] for x in bt["pid"]], case["NI"])
    none = rt.SparseMask.from_lists([[] for _ in range(B)], case["NI"])
    got_m = model.evaluate(seq, seq_len, pos, none, at=(10,))
    want_m = rt.rank_metrics_csr(pos, none, [10], kind="dot", user=net2.user_table(bags), item=net2.V, bias=None, uid=uid)
    assert all(np.array_equal(got_m[k], want_m[k]) for k in ("auc", "ndcg", "recall"))
