"""GPU: the history-pooled recommender with a dense tower (`rt.DeepSeqRec`, `YouTubeRec`, `VanillaYouTubeRec(hidden=...)`) against
tests/tower_ref.py in float64, rounded to float32 once.  The cases are tests/tower_cases.py's (the relu margin holds on each);
tolerances are the project's: conftest.delta_check on tables, TOL on loss and l2, TOL_ADAM on Adam's tables and slots; row
losses stay within fullsoftmax_ref.row_bound_q evaluated on the float64 queries."""
import numpy as np
import pytest

import fullsoftmax_ref as fr
import tower_cases as tc
import tower_ref as tr
from conftest import TOL, TOL_ADAM, delta_check, rel_err

pytestmark = pytest.mark.gpu

_MODELS = {}


def _rt():
    from openrec_amd import runtime as rt
    return rt


def _model(case):
    """the case's model and lists: built once (the seed search of tests/tower_cases.py), shared, never written"""
    if case["name"] not in _MODELS:
        _MODELS[case["name"]] = tc.make(case)
    return _MODELS[case["name"]]


def _dev_opt(rt, name):
    lr = tc.LR[name]
    return {"sgd": lambda: rt.Optimizer.sgd(lr), "adagrad": lambda: rt.Optimizer.adagrad(lr), "adam": lambda: rt.Optimizer.adam(lr),
            "momentum": lambda: rt.Optimizer.momentum(lr, 0.9, True)}[name]()


def _named(m):
    """(name, oracle key, array) of every table of a model"""
    out = [("history", "H", m["H"]), ("item", "V", m["V"]), ("bias", "b", m["b"])]
    out += [(f"side{j}", f"S{j}", s) for j, s in enumerate(m["S"])]
    for l, (W, c) in enumerate(m["layers"]):
        out += [(f"W{l}", f"W{l}", W), (f"c{l}", f"c{l}", c)]
    return [x for x in out if x[2] is not None]


class Net:
    """a model's tables on the device and the rt.DeepSeqRec over them"""

    def __init__(self, m, relu_last, pool="mean"):
        rt = _rt()
        T = lambda x: None if x is None else rt.Table(*x.shape).write(x)
        self.H, self.V, self.b = T(m["H"]), T(m["V"]), T(m["b"])
        self.S = [T(s) for s in m["S"]]
        self.layers = [(T(W), T(c)) for W, c in m["layers"]]
        self.net = rt.DeepSeqRec(self.H, self.V, self.b, self.layers, side=self.S, pool=pool, relu_last=relu_last)

    def tables(self):
        out = [self.H, self.V, self.b] + self.S
        for W, c in self.layers:
            out += [W, c]
        return [t for t in out if t is not None]

    def bits(self):
        return [t.read().view(np.int32) for t in self.tables()]


def _dev(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() if x is not None else None for x in arrays)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _same_losses(a, b):
    return all(np.array_equal(np.asarray(x, np.float32).view(np.int32), np.asarray(y, np.float32).view(np.int32)) for x, y in zip(a, b))


def _extras(case):
    rng = np.random.default_rng(case["seed"] + 100)
    w = rng.uniform(0, 2, case["B"]).astype(np.float32); w[::5] = 0.0
    return w, rng.normal(0, 1, case["NI"]).astype(np.float32)


def _lists(m, device):
    bags, pid, f = (m["ptr"], m["items"]), m["pid"], tuple(m["f"])
    if device:
        bags, (pid,), f = _dev(*bags), _dev(pid), _dev(*f)
    return bags, pid, f


def _step(case, device=False, train=None, want_loss=True, extras=True, scale=2.0, l2_reg=0.01, l2_mlp=0.02):
    """one step of the case on fresh tables -> (Net, optimizer, losses)"""
    rt = _rt()
    m = _model(case)
    n = Net(m, case["relu_last"])
    opt = _dev_opt(rt, case["opt"])
    w, off = _extras(case) if extras else (None, None)
    bags, pid, f = _lists(m, device)
    dw, doff = _dev(w, off) if device else (w, off)
    losses = n.net.step_full(opt, bags, pid, f, weights=dw, item_offset=doff, scale=scale, l2_reg=l2_reg, l2_mlp=l2_mlp, train=train,
                             chunk_items=case["chunk_items"], chunk_samples=case["chunk_samples"], want_loss=want_loss)
    return n, opt, losses


def _reference_step(case, train=tr.ROLES, extras=True, scale=2.0, l2_reg=0.01, l2_mlp=0.02):
    m = _model(case)
    e = tc.copy_model(m, np.float64)
    w, off = _extras(case) if extras else (None, None)
    oo = tc.make_opt(case["opt"])
    want = tr.step(e["H"], e["V"], e["b"], e["S"], e["layers"], m["ptr"], m["items"], m["f"], m["pid"], oo, "mean", case["relu_last"],
                   tc.f64(w), tc.f64(off), scale, float(np.float32(l2_reg)), float(np.float32(l2_mlp)), train)
    return e, oo, want


# ---- 1. one step per case against the float64 reference ----------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", tc.CASES, ids=[c["name"] for c in tc.CASES])
def test_step_matches_the_float64_reference(case, device):
    """every table through delta_check (Adam: TOL_ADAM), W_l, c_l and S_j included; the slots of the dense-applied tables under
    Adam; loss and l2 through TOL.  Weights (some 0), item offsets, scale 2, both l2 coefficients"""
    m = _model(case)
    n, opt, losses = _step(case, device)
    e, oo, want = _reference_step(case)
    print(f"{case['name']}: loss {losses[0][0]:.8g} want {want[0]:.8g}  l2 {losses[1][0]:.8g} want {want[1]:.8g}")
    assert abs(losses[0][0] - want[0]) <= TOL * abs(want[0]) and abs(losses[1][0] - want[1]) <= TOL * abs(want[1])
    for (name, key, W0), t, (_, _, w64) in zip(_named(m), n.tables(), _named(e)):
        got, w32 = t.read(), w64.astype(np.float32)
        print(f"{case['name']} {name}: rel err {rel_err(got, w32):.3g}")
        assert np.isfinite(got).all(), name
        if case["opt"] == "adam":
            assert rel_err(got, w32) <= TOL_ADAM, name
            if name[0] in "ibWc":                 # the slots of the dense-applied tables
                for slot, ref in ((0, oo.m[key]), (1, oo.v[key])):
                    s = np.asarray(opt.slot(t, slot)).reshape(ref.shape)
                    assert rel_err(s, ref.astype(np.float32)) <= TOL_ADAM, (name, slot)
        else:
            delta_check(W0, got, w32, steps=1, what=f"{case['name']} {name}")


def test_host_and_device_lists_give_the_same_bits():
    for case in (tc.CASES[0], tc.CASES[10]):
        a, _, la = _step(case, False)
        c, _, lc = _step(case, True)
        assert _same(a.bits(), c.bits()) and _same_losses(la, lc)


# ---- 2. the forward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(tc.SHAPES)))
def test_loss_full_is_the_steps_loss_bit_for_bit_and_every_row_is_within_the_bound(si):
    case = tc.shape_case(si)
    m = _model(case)
    w, off = _extras(case)
    n = Net(m, case["relu_last"])
    before = n.bits()
    bags, pid, f = _lists(m, False)
    kw = dict(weights=w, item_offset=off, scale=2.0, chunk_items=case["chunk_items"])
    fwd = n.net.loss_full(bags, pid, f, per_row=True, **kw)
    assert _same(before, n.bits())
    dbags, dpid, df = _lists(m, True)
    dw, doff = _dev(w, off)
    fwd_dev = n.net.loss_full(dbags, dpid, df, weights=dw, item_offset=doff, scale=2.0, chunk_items=case["chunk_items"], per_row=True)
    assert fwd_dev[:2] == fwd[:2] and np.array_equal(fwd_dev[2].view(np.int32), fwd[2].view(np.int32))
    losses = n.net.step_full(_dev_opt(_rt(), "sgd"), bags, pid, f, l2_reg=0.01, l2_mlp=0.02, chunk_samples=case["chunk_samples"], **kw)
    assert _same_losses(fwd[:2], (losses[0][0], losses[1][0]))
    e = tc.copy_model(m, np.float64)
    q64 = tr.queries(e["H"], e["S"], e["layers"], m["ptr"], m["items"], m["f"], "mean", case["relu_last"])
    want = fr.row_losses_q(q64, e["V"], e["b"], m["pid"], tc.f64(off), 2.0)
    bound = fr.row_bound_q(q64, e["V"], e["b"], m["pid"], off, 2.0)
    err = np.abs(fwd[2].astype(np.float64) - want)
    print(f"{case['name']}: worst row {(err / bound).max():.3g} x bound; bound {bound.min():.3g} .. {bound.max():.3g}")
    assert fwd[2].shape == (case["B"],) and np.isfinite(fwd[2]).all()
    assert (err <= bound).all(), (int((err > bound).sum()), float((err / bound).max()))


# ---- 3. the anchor to the merged path --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 50])
def test_an_identity_layer_is_seqrec_bit_for_bit(D):
    """no side tables, L = 1, W_0 = I, no bias, relu_last=False: x W is exact in fp32, so the tower is SeqRec -- the row losses, the
    loss and l2 of loss_full, and H, V and b after one SGD step with train=("history", "item", "bias").  D = 64 takes the pool's
    float4 walk, D = 50 the plain one; weights, offsets and l2_reg != 0 ride along"""
    rt = _rt()
    rng = np.random.default_rng(40 + D)
    B, NI = 130, 300
    u = lambda *shape: rng.uniform(-tc.SCALE, tc.SCALE, shape).astype(np.float32)
    H, V, b = u(NI, D), u(NI, D), u(NI, 1)
    ptr, items = tc.fc.make_bags(dict(seed=41, B=B, NI=NI))
    pid = rng.integers(0, NI, B).astype(np.int32)
    w = rng.uniform(0, 2, B).astype(np.float32); off = rng.normal(0, 1, NI).astype(np.float32)
    m = dict(H=H, V=V, b=b, S=[], layers=[[np.eye(D, dtype=np.float32), None]])
    deep = Net(m, relu_last=False)
    T = lambda x: rt.Table(*x.shape).write(x)
    sH, sV, sb = T(H), T(V), T(b)
    seq = rt.SeqRec(sH, sV, sb)
    kw = dict(weights=w, item_offset=off, chunk_items=128)
    a = deep.net.loss_full((ptr, items), pid, per_row=True, **kw)
    c = seq.loss_full((ptr, items), pid, per_row=True, **kw)
    assert _same_losses(a[:2], c[:2]) and np.array_equal(a[2].view(np.int32), c[2].view(np.int32))
    la = deep.net.step_full(rt.Optimizer.sgd(0.05), (ptr, items), pid, l2_reg=0.01, chunk_samples=64, train=("history", "item", "bias"), **kw)
    lc = seq.step_full(rt.Optimizer.sgd(0.05), (ptr, items), pid, l2_reg=0.01, chunk_samples=64, **kw)
    assert _same_losses(la, lc)
    for name, x, y, x0 in (("history", deep.H, sH, H), ("item", deep.V, sV, V), ("bias", deep.b, sb, b)):
        assert np.array_equal(x.read().view(np.int32), y.read().view(np.int32)), name
        assert not np.array_equal(x.read(), x0), name
    assert np.array_equal(deep.layers[0][0].read(), np.eye(D, dtype=np.float32))


# ---- 4. row independence; the queries of user_table are the step's ------------------------------------------------------------------
def test_a_query_row_has_the_same_bits_in_any_batch_and_is_the_row_the_step_scores():
    rt = _rt()
    case = tc.shape_case(0)
    m = _model(case)
    n = Net(m, case["relu_last"])
    Q = n.net.user_table((m["ptr"], m["items"]), tuple(m["f"])).read().copy()
    e = tc.copy_model(m, np.float64)
    q64 = tr.queries(e["H"], e["S"], e["layers"], m["ptr"], m["items"], m["f"], "mean", True)
    assert Q.shape == (130, 50) and rel_err(Q, q64.astype(np.float32)) <= TOL
    k = 65
    first = n.net.user_table((m["ptr"][:k + 1], m["items"][:m["ptr"][k]]), tuple(f[:k] for f in m["f"]), out=rt.Table(k, 50)).read()
    assert np.array_equal(first.view(np.int32), Q[:k].view(np.int32))
    dev = n.net.user_table(_dev(m["ptr"], m["items"]), _dev(*m["f"]), out=rt.Table(130, 50)).read()
    assert np.array_equal(dev.view(np.int32), Q.view(np.int32))
    # the pooled columns are rt.bag_pool's bits: a tower that copies them out (W = [0; I], no bias, linear)
    for Dh in (50, 64):
        rng = np.random.default_rng(Dh)
        H = rng.uniform(-1, 1, (300, Dh)).astype(np.float32)
        S = rng.uniform(-1, 1, (7, 3)).astype(np.float32)
        W = np.concatenate([np.zeros((3, Dh), np.float32), np.eye(Dh, dtype=np.float32)])
        mm = dict(H=H, V=np.zeros((300, Dh), np.float32), b=None, S=[S], layers=[[W, None]])
        nn = Net(mm, relu_last=False)
        bags = (m["ptr"], m["items"])
        got = nn.net.user_table(bags, (rng.integers(0, 7, 130).astype(np.int32),)).read()
        want = rt.bag_pool(nn.H, bags, rt.Table(130, Dh)).read()
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), Dh
    # the step scores with these rows: a one-row batch through the tower, and the same row of user_table through the user-table form
    Qt = rt.Table(130, 50).write(Q)
    for i in (0, 64, 129):                          # bag 0 is empty
        lo, hi = m["ptr"][i], m["ptr"][i + 1]
        one = n.net.loss_full((np.array([0, hi - lo], np.int32), m["items"][lo:hi]), m["pid"][i:i + 1], tuple(f[i:i + 1] for f in m["f"]), per_row=True)
        ref = rt.fullsoftmax_loss(Qt, n.V, n.b, np.array([i], np.int32), m["pid"][i:i + 1], per_row=True)
        assert np.float32(one[0]).view(np.int32) == np.float32(ref[0]).view(np.int32) and np.array_equal(one[2].view(np.int32), ref[2].view(np.int32)), i


# ---- 5. repeatability ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", tc.OPTS)
def test_two_runs_of_a_step_give_the_same_bits_in_every_table(opt):
    case = tc.shape_case(0, opt, seed=7000)
    a, _, la = _step(case)
    c, _, lc = _step(case)
    assert _same(a.bits(), c.bits()) and _same_losses(la, lc)
    d, _, none = _step(case, device=True, want_loss=False)
    assert none is None and _same(a.bits(), d.bits())


# ---- 6. train masks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_train_masks_leave_every_other_table_bit_identical(opt):
    case = tc.shape_case(0, opt, seed=7000)
    m = _model(case)
    names = [x[0] for x in _named(m)]
    role = lambda name: {"h": "history", "i": "item", "b": "bias", "s": "side"}.get(name[0], "tower")
    before = [x[2].view(np.int32) for x in _named(m)]
    for train in (("history",), ("item",), ("bias",), ("side",), ("tower",), ("history", "tower")):
        n, o, _ = _step(case, train=train)
        e, _, _ = _reference_step(case, train=train)
        for name, b0, b1, t, (_, _, W0), (_, _, w64) in zip(names, before, n.bits(), n.tables(), _named(m), _named(e)):
            if role(name) in train:
                assert not np.array_equal(b0, b1), (train, name)
                if opt == "adam":
                    assert rel_err(t.read(), w64.astype(np.float32)) <= TOL_ADAM, (train, name)
                else:
                    delta_check(W0, t.read(), w64.astype(np.float32), steps=1, what=f"mask {train} {name}")
            else:
                assert np.array_equal(b0, b1), (train, name)
                if opt == "adam" and name[0] in "ibWc":
                    assert not any(np.asarray(o.slot(t, s)).any() for s in (0, 1)), (train, name)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_with_messages_before_any_device_work():
    import ctypes
    from openrec_amd import _ffi
    rt = _rt()
    case = tc.shape_case(0)
    m = _model(case)
    n = Net(m, True)
    ctx = n.H.ctx
    before = n.bits()
    sgd = rt.Optimizer.sgd(0.05)
    harr = lambda ts: (ctypes.c_void_p * max(len(ts), 1))(*[None if t is None else t._h for t in ts])
    f = [np.ascontiguousarray(x) for x in m["f"]]

    def raw(H=n.H, V=n.V, b=n.b, S=None, W=None, c=None, opt=sgd, l2_mlp=0.0, mask=0, flags=0):
        S = n.S if S is None else S
        W = [w for w, _ in n.layers] if W is None else W
        c = [x for _, x in n.layers] if c is None else c
        ids = (ctypes.c_void_p * max(len(S), 1))(*[f[j % 2].ctypes.data for j in range(len(S))])
        _ffi.check(ctx._lib.orx_tower_step(ctx._h, opt._h, H._h, V._h, b._h if b is not None else None, len(S), harr(S), ids, len(W), harr(W),
                                           harr(c), 1, m["ptr"].ctypes.data, m["items"].ctypes.data, m["pid"].ctypes.data, None, None, 130,
                                           len(m["items"]), _ffi.ORX_BAG_MEAN, 1.0, 1.0, 0.0, l2_mlp, 0, 0, mask, flags, None, None))
    T = rt.Table
    W0, W1 = n.layers[0][0], n.layers[1][0]
    bad = [(dict(W=[T(58, 257), T(257, 50)], c=[None, None]), "width outside"),
           (dict(H=T(300, 250)), "above 256"),
           (dict(W=[W0, T(70, 40)], c=[None, None]), "the item table has dim"),
           (dict(W=[W0, T(60, 50)], c=[None, None]), "do not chain"),
           (dict(W=[], c=[]), "layers"), (dict(W=[W0, T(70, 70), T(70, 70), T(70, 70), W1], c=[None] * 5), "layers"),
           (dict(S=n.S + [T(2, 1), T(2, 1), T(2, 1)]), "side tables"),
           (dict(S=[n.S[0], n.S[0]]), "passed twice"), (dict(W=[W0, W0]), "passed twice"), (dict(V=n.H), "passed twice"),
           (dict(c=[T(70, 1), None]), "not \\[1, 70\\]"), (dict(c=[n.layers[0][1], T(1, 49)]), "not \\[1, 50\\]"),
           (dict(l2_mlp=-1.0), "l2_mlp"), (dict(l2_mlp=float("nan")), "l2_mlp"), (dict(l2_mlp=0.5, flags=_ffi.ORX_NO_L2), "ORX_NO_L2"),
           (dict(mask=64), "train mask"), (dict(mask=_ffi.ORX_TRAIN_BIAS, b=None), "ORX_TRAIN_BIAS"),
           (dict(flags=_ffi.ORX_HOGWILD), "ORX_HOGWILD"), (dict(b=T(299, 1)), "item_bias"), (dict(V=T(299, 50)), "history rows"),
           (dict(S=[n.S[0], T(37, 5, rt.Context(0))]), "different context")]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            raw(**kw)
    with pytest.raises(ValueError, match="ORX_TRAIN_SIDE"):
        nos = Net(dict(m, S=[], layers=[[np.zeros((50, 50), np.float32), None]]), True)
        _ffi.check(ctx._lib.orx_tower_step(ctx._h, sgd._h, nos.H._h, nos.V._h, None, 0, harr([]), harr([]), 1, harr([nos.layers[0][0]]), None, 1,
                                           m["ptr"].ctypes.data, m["items"].ctypes.data, m["pid"].ctypes.data, None, None, 130, len(m["items"]),
                                           _ffi.ORX_BAG_MEAN, 1.0, 1.0, 0.0, 0.0, 0, 0, _ffi.ORX_TRAIN_SIDE, 0, None, None))
    ctx.synchronize()
    assert _same(before, n.bits())
    raw()                                       # and the call as it stands is accepted
    assert not _same(before, n.bits())


def test_a_side_id_out_of_range_raises_and_leaves_the_good_samples_alone():
    """device lists: the call raises IndexError, the good samples' row losses keep their bits, the tables match the reference with
    the bad sample removed (weights (B - 1) / B keep c_i = 1 / B), and the next call succeeds"""
    rt = _rt()
    case = tc.shape_case(0)
    m = _model(case)
    n = Net(m, True)
    bags, pid, f = _lists(m, False)
    good = n.net.loss_full(bags, pid, f, chunk_items=128, per_row=True)[2]
    k = 71
    fbad = [x.copy() for x in m["f"]]; fbad[1][k] = 37
    keep = np.arange(130) != k
    with pytest.raises(IndexError):
        n.net.loss_full(_dev(*bags), *_dev(pid), _dev(*fbad), chunk_items=128)
    rows = n.net.loss_full(bags, pid, f, chunk_items=128, per_row=True)[2]
    assert np.array_equal(rows.view(np.int32), good.view(np.int32))
    with pytest.raises(IndexError):
        n.net.step_full(rt.Optimizer.sgd(0.05), _dev(*bags), *_dev(pid), _dev(*fbad), l2_reg=0.01, l2_mlp=0.02, chunk_items=128, chunk_samples=64)
    assert all(np.isfinite(t.read()).all() for t in n.tables())
    e = tc.copy_model(m, np.float64)
    lo, hi = m["ptr"][k], m["ptr"][k + 1]
    ptr2 = np.concatenate([m["ptr"][:k + 1], m["ptr"][k + 2:] - (hi - lo)])
    items2 = np.concatenate([m["items"][:lo], m["items"][hi:]])
    tr.step(e["H"], e["V"], e["b"], e["S"], e["layers"], ptr2, items2, [x[keep] for x in m["f"]], m["pid"][keep], tc.make_opt("sgd"), "mean",
            True, np.full(129, 129.0 / 130.0), None, 1.0, float(np.float32(0.01)), float(np.float32(0.02)))
    for (name, _, W0), t, (_, _, w64) in zip(_named(m), n.tables(), _named(e)):
        delta_check(W0, t.read(), w64.astype(np.float32), steps=1, what=f"side id out of range, {name}")
    with pytest.raises(IndexError):
        n.net.user_table(bags, tuple(fbad))
    _step(case)


# ---- 8. the tf2 layer ---------------------------------------------------------------------------------------------------------------
def _padded(m, L):
    lens = np.diff(m["ptr"]).astype(np.int32)
    seq = np.zeros((len(lens), L), np.int32)
    for i, k in enumerate(lens):
        seq[i, :k] = m["items"][m["ptr"][i]:m["ptr"][i + 1]]
    return seq, lens


def test_youtube_rec_is_the_runtime_call():
    rt = _rt()
    from openrec_amd.tf2.recommenders import YouTubeRec
    case = tc.shape_case(0)
    m = _model(case)
    L = 6
    seq, lens = _padded(m, L)
    model = YouTubeRec(user_dict={"gender": 2, "geo": 37}, item_dict={"id": 300}, dim_user_embed={"gender": 3, "geo": 5, "total": 8},
                       dim_item_embed={"id": 50, "total": 50}, max_seq_len=L, l2_reg_embed=0.01, l2_reg_mlp=0.02, hidden=[70, 50], use_item_bias=True)
    ref = YouTubeRec({"gender": 2, "geo": 37}, {"id": 300}, {"gender": 3, "geo": 5, "total": 8}, {"id": 50, "total": 50}, L)
    assert ref.item_latent_factor.table.shape == (300, 58) and [w.table.shape for w in ref.mlp_weights] == [(58, 58)] and ref.item_bias is None
    a = np.sqrt(6.0 / 116)
    W = ref.mlp_weights[0].table.read()
    assert np.abs(W).max() <= a and np.abs(W).max() > 0.9 * a and not ref.mlp_biases[0].table.read().any()
    model.seq_item_latent_factor.table.write(m["H"]); model.item_latent_factor.table.write(m["V"]); model.item_bias.table.write(m["b"])
    for lf, s in zip(model.user_feature_factors, m["S"]):
        lf.table.write(s)
    for Wl, cl, (W, c) in zip(model.mlp_weights, model.mlp_biases, m["layers"]):
        Wl.table.write(W); cl.table.write(c)
    feats = dict(gender=m["f"][0], geo=m["f"][1])
    fwd = model.loss_full(seq, lens, m["pid"], **feats)
    got = model.train_steps_full(rt.Optimizer.adam(0.002), seq, lens, m["pid"], **feats)
    n = Net(m, True, pool=("fixed", L))
    want = n.net.step_full(rt.Optimizer.adam(0.002), (m["ptr"], m["items"]), m["pid"], tuple(m["f"]), l2_reg=0.01, l2_mlp=0.02)
    assert _same_losses(got, want) and np.float32(fwd[0]).view(np.int32) == got[0].view(np.int32)[0]
    mine = [model.seq_item_latent_factor, model.item_latent_factor, model.item_bias, *model.user_feature_factors]
    for Wl, cl in zip(model.mlp_weights, model.mlp_biases):
        mine += [Wl, cl]
    assert _same([lf.table.read().view(np.int32) for lf in mine], n.bits())
    ids, scores = model.recommend(seq, lens, 7, **feats)
    wi, ws = rt.recommend_topk("dot", n.net.user_table((m["ptr"], m["items"]), tuple(m["f"])), n.V, n.b, np.arange(130, dtype=np.int32), 7)
    assert np.array_equal(np.asarray(ids), np.asarray(wi)) and np.array_equal(np.asarray(scores), np.asarray(ws))
    assert np.asarray(model.inference(seq, lens, **feats)).shape == (130, 300)
    with pytest.raises(ValueError):
        model.train_steps_full(rt.Optimizer.sgd(0.05), seq, lens, m["pid"], gender=m["f"][0])
    with pytest.raises(NotImplementedError):
        model.train_steps(rt.Optimizer.sgd(0.05), seq, lens, m["pid"], np.zeros((130, 2), np.int32))


def test_vanilla_youtube_rec_with_hidden_layers_is_the_runtime_call():
    rt = _rt()
    from openrec_amd.tf2.recommenders import VanillaYouTubeRec
    case = tc.shape_case(4)                           # no side tables: 24 -> 24
    m = _model(case)
    L = 6
    seq, lens = _padded(m, L)
    model = VanillaYouTubeRec(24, L, 300, l2_reg_embed=0.01, use_item_bias=False, hidden=[24], l2_reg_mlp=0.02)
    assert VanillaYouTubeRec(24, L, 300)._deep is False
    model.seq_item_latent_factor.table.write(m["H"]); model.item_latent_factor.table.write(m["V"])
    model.mlp_weights[0].table.write(m["layers"][0][0]); model.mlp_biases[0].table.write(m["layers"][0][1])
    got = model.train_steps_full(rt.Optimizer.adagrad(0.05), seq, lens, m["pid"])
    n = Net(m, True, pool=("fixed", L))               # (the tf2 layers are Dense + bias + relu)
    want = n.net.step_full(rt.Optimizer.adagrad(0.05), (m["ptr"], m["items"]), m["pid"], l2_reg=0.01, l2_mlp=0.02)
    assert _same_losses(got, want)
    mine = [model.seq_item_latent_factor, model.item_latent_factor, model.mlp_weights[0], model.mlp_biases[0]]
    assert _same([lf.table.read().view(np.int32) for lf in mine], n.bits())
    ids, scores = model.recommend(seq, lens, 5)
    wi, ws = n.net.recommend((m["ptr"], m["items"]), (), 5)
    assert np.array_equal(np.asarray(ids), np.asarray(wi)) and np.array_equal(np.asarray(scores), np.asarray(ws))
    assert np.asarray(model.inference(seq, lens)).shape == (65, 300)
