"""GPU: training on label sets under the full softmax (`rt.SeqRec.step_full(labels=...)`, `rt.DeepSeqRec.step_full(labels=...)`,
`VanillaYouTubeRec.train_steps_sets`, `MultDAE.train_steps`) against tests/labelsets_ref.py in float64, rounded to float32 once.
The sets are tests/labelsets_cases.py's on the shapes of tests/fullsoftmax_cases.py (the SeqRec form) and tests/tower_cases.py
(the tower form); the per-row bound is labelsets_ref.row_bound_q, whose headroom tests/test_labelsets_cpu.py shows.  Tolerances are
the project's: conftest.delta_check on tables, TOL on loss and l2, TOL_ADAM on Adam's tables and slots."""
import numpy as np
import pytest

import fullsoftmax_cases as fc
import labelsets_cases as lc
import labelsets_ref as lr
import seqrec_ref as sr
import tower_cases as tc
import tower_ref as tr
from conftest import TOL, TOL_ADAM, delta_check, rel_err

pytestmark = pytest.mark.gpu

MID = dict(opt="sgd", bias=True, B=130, D=50, NU=200, NI=300, chunk_items=128, chunk_samples=64, seed=78, name="mid")
_TOWER = {}


def _rt():
    from openrec_amd import runtime as rt
    return rt


def _dev_opt(rt, name):
    lr_ = fc.LR[name]
    return {"sgd": lambda: rt.Optimizer.sgd(lr_), "adagrad": lambda: rt.Optimizer.adagrad(lr_), "adam": lambda: rt.Optimizer.adam(lr_),
            "momentum": lambda: rt.Optimizer.momentum(lr_, 0.9, True)}[name]()


def _tables(rt, *arrays):
    return tuple(rt.Table(*x.shape).write(x) if x is not None else None for x in arrays)


def _dev(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() if x is not None else None for x in arrays)


def _bits(*tables):
    return [t.read().view(np.int32) for t in tables if t is not None]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _same_losses(a, b):
    return all(np.array_equal(np.asarray(x, np.float32).view(np.int32), np.asarray(y, np.float32).view(np.int32)) for x, y in zip(a, b))


def _f64(x):
    return None if x is None else np.asarray(x).astype(np.float64)


def _extras(case, minus_inf=None):
    """sample weights (some 0) and item offsets; minus_inf: the label items, one item outside of which goes to -inf"""
    rng = np.random.default_rng(case["seed"] + 100)
    w = rng.uniform(0, 2, case["B"]).astype(np.float32); w[::5] = 0.0
    off = rng.normal(0, 1, case["NI"]).astype(np.float32)
    if minus_inf is not None:
        free = np.setdiff1d(np.arange(case["NI"]), minus_inf)
        if len(free):
            off[free[len(free) // 2]] = -np.inf
    return w, off


def _check_tables(what, optname, names, orig, got_tabs, want):
    for name, W0, t, w in zip(names, orig, got_tabs, want):
        if t is None:
            continue
        got, w32 = t.read(), w.astype(np.float32)
        print(f"{what} {name}: rel err {rel_err(got, w32):.3g}")
        assert np.isfinite(got).all(), (what, name)
        if optname == "adam":
            assert rel_err(got, w32) <= TOL_ADAM, (what, name)
        else:
            delta_check(W0, got, w32, steps=1, what=f"{what} {name}")


def _check_losses(what, losses, want):
    print(f"{what}: loss {losses[0][0]:.8g} want {want[0]:.8g}  l2 {losses[1][0]:.8g} want {want[1]:.8g}")
    assert abs(losses[0][0] - want[0]) <= TOL * abs(want[0]) and abs(losses[1][0] - want[1]) <= TOL * abs(want[1]), what


def _check_rows(what, rows, want, bound):
    err = np.abs(rows.astype(np.float64) - want)
    live = bound > 0
    ratio = (err[live] / bound[live]).max() if live.any() else 0.0
    print(f"{what}: worst row {ratio:.3g} x bound; bound {bound[live].min() if live.any() else 0:.3g} .. {bound.max():.3g}")
    assert rows.shape == want.shape and np.isfinite(rows).all()
    assert (err <= bound).all(), (what, int((err > bound).sum()), float(ratio))


# ---- the SeqRec form -----------------------------------------------------------------------------------------------------------------
def _seq_step(case, lists=None, lw=None, w=None, off=None, scale=2.0, l2_reg=0.01, train=None, want_loss=True, pool="mean", how="host"):
    """one step on fresh tables -> (the case's arrays, tables, optimizer, losses)"""
    rt = _rt()
    H, V, b, ptr, items = lc.make_seq(case)
    lptr, litems = lists if lists is not None else lc.make_sets(case)[:2]
    tabs = _tables(rt, H, V, b)
    opt = _dev_opt(rt, case["opt"])
    bags, labels, a_lw, a_w, a_off = (ptr, items), (lptr, litems), lw, w, off
    if how == "device":
        bags, labels, (a_lw, a_w, a_off) = _dev(ptr, items), _dev(lptr, litems), _dev(lw, w, off)
    elif how == "padded":
        bags, labels = lc.padded(ptr, items), lc.padded(lptr, litems)
        if lw is not None:
            a_lw = np.zeros(labels[0].shape, np.float32)
            a_lw[np.arange(labels[0].shape[1])[None, :] < labels[1][:, None]] = lw
    losses = rt.SeqRec(*tabs, pool=pool).step_full(opt, bags, None, weights=a_w, item_offset=a_off, scale=scale, l2_reg=l2_reg, train=train,
                                                   chunk_items=case["chunk_items"], chunk_samples=case["chunk_samples"], want_loss=want_loss,
                                                   labels=labels, label_weights=a_lw)
    return (H, V, b, ptr, items, lptr, litems), tabs, opt, losses


def _seq_reference(case, arrays, lw=None, w=None, off=None, scale=2.0, l2_reg=0.01, train=("history", "item", "bias"), pool="mean"):
    H, V, b, ptr, items, lptr, litems = arrays
    e = [_f64(H), _f64(V), _f64(b)]
    oo = fc.make_opt(case["opt"])
    want = lr.seq_step(*e, ptr, items, lptr, litems, oo, pool, _f64(lw), _f64(w), _f64(off), scale, float(np.float32(l2_reg)), train)
    return e, oo, want


@pytest.mark.parametrize("case", fc.CASES, ids=[c["name"] for c in fc.CASES])
def test_seqrec_step_matches_the_float64_reference(case):
    """the four optimizers x with / without the bias on every shape: every table, the losses, Adam's slots of the dense-applied
    tables.  Label weights, sample weights (some 0), item offsets, scale 2, l2_reg 0.01"""
    lptr, litems, lw = lc.make_sets(case, weights=True)
    w, off = _extras(case)
    arrays, tabs, opt, losses = _seq_step(case, (lptr, litems), lw, w, off)
    e, oo, want = _seq_reference(case, arrays, lw, w, off)
    _check_tables(case["name"], case["opt"], ("history", "item", "bias"), arrays[:3], tabs, e)
    _check_losses(case["name"], losses, want)
    if case["opt"] == "adam":
        for name, t, key in (("item", tabs[1], "V"), ("bias", tabs[2], "b")):
            if t is not None:
                for slot, ref in ((0, oo.m[key]), (1, oo.v[key])):
                    assert rel_err(np.asarray(opt.slot(t, slot)).reshape(ref.shape), ref.astype(np.float32)) <= TOL_ADAM, (name, slot)


@pytest.mark.parametrize("si", range(len(fc.SHAPES)))
@pytest.mark.parametrize("bias,offset,weights", [(True, True, True), (False, False, False), (True, False, True), (False, True, False)])
def test_seqrec_every_row_loss_is_within_the_bound(si, bias, offset, weights):
    rt = _rt()
    case = fc.shape_case(si, bias=bias, seed=500 + si)
    H, V, b, ptr, items = lc.make_seq(case)
    lptr, litems, lw = lc.make_sets(case, weights)
    w, off = _extras(case, minus_inf=litems)
    off = off if offset else None
    net = rt.SeqRec(*_tables(rt, H, V, b))
    Q64, _ = sr.pool_rows(_f64(H), ptr, items, "mean")
    for scale in (1.0, 4.0):
        loss, l2, rows = net.loss_full((ptr, items), weights=w, item_offset=off, scale=scale, chunk_items=case["chunk_items"], per_row=True,
                                       labels=(lptr, litems), label_weights=lw)
        want = lr.row_losses_q(Q64, _f64(V), _f64(b), lptr, litems, _f64(lw), _f64(off), scale)
        bound = lr.row_bound_q(Q64, _f64(V), _f64(b), lptr, litems, _f64(lw), off, scale)
        _check_rows(f"{case['name']} scale={scale}", rows, want, bound)
        mean = float(np.mean(_f64(w) * want))
        assert abs(loss - mean) <= TOL * abs(mean)


@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_seqrec_train_masks_leave_the_other_tables_and_their_slots_untouched(opt):
    case = dict(MID, opt=opt, name=f"mask-{opt}")
    H, V, b, _, _ = lc.make_seq(case)
    before = [x.view(np.int32) for x in (H, V, b)]
    arrays, tabs, o, _ = _seq_step(case, train=("history",))
    after = _bits(*tabs)
    assert np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2]) and not np.array_equal(before[0], after[0])
    if opt == "adam":
        assert all(not np.asarray(o.slot(t, s)).any() for t in tabs[1:] for s in (0, 1))
    e, _, _ = _seq_reference(case, arrays, train=("history",))
    _check_tables("history alone", opt, ("history",), arrays[:1], tabs[:1], e[:1])
    arrays, tabs, o, _ = _seq_step(case, train=("item", "bias"))
    after = _bits(*tabs)
    assert np.array_equal(before[0], after[0]) and not np.array_equal(before[1], after[1]) and not np.array_equal(before[2], after[2])
    e, _, _ = _seq_reference(case, arrays, train=("item", "bias"))
    _check_tables("item and bias", opt, ("history", "item", "bias"), arrays[:3], tabs, e)
    _, tabs, _, _ = _seq_step(case, train=("bias",))
    after = _bits(*tabs)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and not np.array_equal(before[2], after[2])


@pytest.mark.parametrize("si", [3, 4, 7])
def test_the_forward_is_the_steps_loss_bit_for_bit_and_changes_nothing(si):
    rt = _rt()
    case = fc.shape_case(si)
    H, V, b, ptr, items = lc.make_seq(case)
    lptr, litems, lw = lc.make_sets(case, weights=True)
    w, off = _extras(case)
    tabs = _tables(rt, H, V, b)
    net = rt.SeqRec(*tabs)
    before = _bits(*tabs)
    kw = dict(weights=w, item_offset=off, scale=2.0, chunk_items=case["chunk_items"], labels=(lptr, litems), label_weights=lw)
    fwd = net.loss_full((ptr, items), per_row=True, **kw)
    assert _same(before, _bits(*tabs))
    dw, doff, dlw = _dev(w, off, lw)
    fwd_dev = net.loss_full(_dev(ptr, items), weights=dw, item_offset=doff, scale=2.0, chunk_items=case["chunk_items"], per_row=True,
                            labels=_dev(lptr, litems), label_weights=dlw)
    losses = net.step_full(_dev_opt(rt, "sgd"), (ptr, items), l2_reg=0.01, chunk_samples=case["chunk_samples"], **kw)
    assert _same_losses(fwd[:2], (losses[0][0], losses[1][0]))
    assert fwd_dev[:2] == fwd[:2] and np.array_equal(fwd_dev[2].view(np.int32), fwd[2].view(np.int32))
    assert not _same(before, _bits(*tabs))


@pytest.mark.parametrize("opt", fc.OPTS)
def test_two_runs_of_a_step_give_the_same_bits_in_every_table_and_row_loss(opt):
    """the item every set holds is one run of the item side that every sample is in; sets repeat items"""
    rt = _rt()
    case = dict(MID, opt=opt)
    lptr, litems, lw = lc.make_sets(case, weights=True)
    w, off = _extras(case)
    _, a, _, la = _seq_step(case, (lptr, litems), lw, w, off)
    arrays, c, _, lc_ = _seq_step(case, (lptr, litems), lw, w, off)
    assert _same(_bits(*a), _bits(*c)) and _same_losses(la, lc_)
    H, V, b, ptr, items = arrays[:5]
    rows = [rt.SeqRec(*_tables(rt, H, V, b)).loss_full((ptr, items), labels=(lptr, litems), label_weights=lw, per_row=True)[2] for _ in range(2)]
    assert np.array_equal(rows[0].view(np.int32), rows[1].view(np.int32))


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
def test_sets_of_one_with_unit_weights_against_the_single_label_step(opt):
    """equal to fp32 rounding, not bit for bit: from the same start, the single-label tables are the `want` of delta_check"""
    rt = _rt()
    case = dict(MID, opt=opt)
    H, V, b, ptr, items = lc.make_seq(case)
    pid = fc.make(case)[4]
    w, off = _extras(case)
    kw = dict(weights=w, item_offset=off, scale=2.0, l2_reg=0.01, chunk_items=128, chunk_samples=64)
    a = _tables(rt, H, V, b)
    la = rt.SeqRec(*a).step_full(_dev_opt(rt, opt), (ptr, items), pid, **kw)
    c = _tables(rt, H, V, b)
    lc_ = rt.SeqRec(*c).step_full(_dev_opt(rt, opt), (ptr, items), labels=(np.arange(case["B"] + 1, dtype=np.int32), pid), **kw)
    assert abs(la[0][0] - lc_[0][0]) <= TOL * abs(la[0][0]) and abs(la[1][0] - lc_[1][0]) <= TOL * abs(la[1][0])
    for name, W0, x, y in zip(("history", "item", "bias"), (H, V, b), a, c):
        delta_check(W0, y.read(), x.read(), steps=1, what=f"sets of one, {name}")


def test_a_sample_with_an_empty_set_moves_no_item_row_and_keeps_its_l2_part():
    """the batch with sample k's set emptied against the batch with sample k at weight 0 and sets of the other samples as they
    were: SGD moves the item table and the bias by the same bits (the empty sample adds exactly nothing to them); its history
    rows move by its l2 part alone, which the reference holds; l2_out keeps |q_k|^2 / 2"""
    rt = _rt()
    case = dict(MID, name="empty")
    lens = lc.set_lens(case)
    k = 4
    assert lens[k] > 0
    lens[k] = 0
    lptr, litems, _ = lc.make_sets(case, lens=lens)
    arrays, tabs, _, losses = _seq_step(case, (lptr, litems), l2_reg=0.05)
    e, _, want = _seq_reference(case, arrays, l2_reg=0.05)
    _check_tables("empty set", "sgd", ("history", "item", "bias"), arrays[:3], tabs, e)
    _check_losses("empty set", losses, want)
    w0 = np.ones(case["B"], np.float32); w0[k] = 0.0
    _, tabs0, _, _ = _seq_step(case, (lptr, litems), w=w0, l2_reg=0.05)
    assert _same(_bits(*tabs[1:]), _bits(*tabs0[1:]))
    H, V, b, ptr, items = arrays[:5]
    rows = rt.SeqRec(*_tables(rt, H, V, b)).loss_full((ptr, items), labels=(lptr, litems), per_row=True)[2]
    assert rows[k] == 0.0 and (rows[np.diff(lptr) > 0] > 0).all()


@pytest.mark.parametrize("D", [3, 64])
def test_a_bad_id_in_a_label_set_raises_and_leaves_the_good_samples_alone(D):
    """the prepare pass's own bounds check (no id is ever an address): the call raises, the good samples' row losses are those of
    the call without the bad id bit for bit, the bad sample's is 0, the step's tables match the reference without the sample
    (weights (B - 1) / B keep c_i = 1 / B), a malformed device lab_ptr raises too, and the next call succeeds"""
    rt = _rt()
    from openrec_amd import _ffi
    case = dict(MID, D=D, name=f"bad-label-D{D}")
    B = case["B"]
    H, V, b, ptr, items = lc.make_seq(case)
    lptr, litems, _ = lc.make_sets(case)
    tabs = _tables(rt, H, V, b)
    net = rt.SeqRec(*tabs)
    good = net.loss_full((ptr, items), labels=(lptr, litems), chunk_items=128, per_row=True)[2]
    k = 70
    assert lptr[k + 1] - lptr[k] >= 65
    bad = litems.copy(); bad[lptr[k] + 64] = case["NI"]                 # in the second 64-id load of the set
    keep = np.arange(B) != k
    import torch
    rows = torch.zeros(B, dtype=torch.float32, device="cuda")
    ctx = tabs[0].ctx
    dp, di, dlp, dli = _dev(ptr, items, lptr, bad)
    ctx.after_torch(dp, di, dlp, dli, rows)
    with pytest.raises(IndexError):
        _ffi.check(ctx._lib.orx_seqrec_full_sets_loss(ctx._h, tabs[0]._h, tabs[1]._h, tabs[2]._h, dp.data_ptr(), di.data_ptr(), dlp.data_ptr(),
                                                      dli.data_ptr(), None, len(bad), None, None, B, len(items), _ffi.ORX_BAG_MEAN, 0.0, 1.0, 128,
                                                      _ffi.ORX_IDS_DEVICE, None, None, rows.data_ptr()))
    rows = rows.cpu().numpy()
    assert np.array_equal(rows[keep].view(np.int32), good[keep].view(np.int32)) and rows[k] == 0.0
    with pytest.raises(IndexError):
        net.step_full(_dev_opt(rt, "sgd"), (ptr, items), labels=(lptr, bad), l2_reg=0.01, chunk_items=128, chunk_samples=64)
    assert all(np.isfinite(t.read()).all() for t in tabs)
    # the reference without sample k: its bag and its set removed
    bl, ll = np.diff(ptr), np.diff(lptr)
    ptr2 = np.concatenate([[0], np.cumsum(bl[keep])]).astype(np.int32)
    lptr2 = np.concatenate([[0], np.cumsum(ll[keep])]).astype(np.int32)
    items2 = np.concatenate([items[ptr[i]:ptr[i + 1]] for i in np.flatnonzero(keep)]).astype(np.int32)
    litems2 = np.concatenate([litems[lptr[i]:lptr[i + 1]] for i in np.flatnonzero(keep)]).astype(np.int32)
    e = [_f64(H), _f64(V), _f64(b)]
    lr.seq_step(*e, ptr2, items2, lptr2, litems2, fc.make_opt("sgd"), "mean", w=np.full(B - 1, (B - 1.0) / B), l2_reg=float(np.float32(0.01)))
    _check_tables("label out of range", "sgd", ("history", "item", "bias"), (H, V, b), tabs, e)
    neg = litems.copy(); neg[lptr[1]] = -1
    with pytest.raises(IndexError):
        net.loss_full((ptr, items), labels=(lptr, neg))
    dec = lptr.copy(); dec[5] = dec[4] - 1
    with pytest.raises(ValueError):
        net.step_full(_dev_opt(rt, "sgd"), (ptr, items), labels=(dec, litems))
    with pytest.raises(IndexError):
        net.step_full(_dev_opt(rt, "sgd"), _dev(ptr, items), labels=_dev(dec, litems))
    assert all(np.isfinite(t.read()).all() for t in tabs)
    tabs = _tables(rt, H, V, b)
    again = rt.SeqRec(*tabs).loss_full((ptr, items), labels=(lptr, litems), chunk_items=128, per_row=True)[2]
    assert np.array_equal(again.view(np.int32), good.view(np.int32))


@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_ragged_device_padded_host_and_ragged_host_lists_give_the_same_bits(opt):
    case = dict(MID, opt=opt)
    lptr, litems, lw = lc.make_sets(case, weights=True)
    w, off = _extras(case)
    runs = [_seq_step(case, (lptr, litems), lw, w, off, how=how) for how in ("host", "device", "padded")]
    for _, tabs, _, losses in runs[1:]:
        assert _same(_bits(*runs[0][1]), _bits(*tabs)) and _same_losses(runs[0][3], losses)
    _, tabs, _, none = _seq_step(case, (lptr, litems), lw, w, off, how="device", want_loss=False)
    assert none is None and _same(_bits(*runs[0][1]), _bits(*tabs))


# ---- the tower form ------------------------------------------------------------------------------------------------------------------
def _tower_model(case):
    if case["name"] not in _TOWER:
        m = tc.make(case)
        m["lptr"], m["litems"], m["lw"] = lc.make_sets(dict(seed=case["seed"], B=case["B"], NI=case["NI"]), weights=True)
        _TOWER[case["name"]] = m
    return _TOWER[case["name"]]


class Net:
    """a model's tables on the device and the rt.DeepSeqRec over them"""

    def __init__(self, m, relu_last):
        rt = _rt()
        T = lambda x: None if x is None else rt.Table(*x.shape).write(x)
        self.H, self.V, self.b = T(m["H"]), T(m["V"]), T(m["b"])
        self.S = [T(s) for s in m["S"]]
        self.layers = [(T(W), T(c)) for W, c in m["layers"]]
        self.net = rt.DeepSeqRec(self.H, self.V, self.b, self.layers, side=self.S, pool="mean", relu_last=relu_last)

    def tables(self):
        out = [self.H, self.V, self.b] + self.S
        for W, c in self.layers:
            out += [W, c]
        return [t for t in out if t is not None]


def _named(m):
    out = [("history", "H", m["H"]), ("item", "V", m["V"]), ("bias", "b", m["b"])]
    out += [(f"side{j}", f"S{j}", s) for j, s in enumerate(m["S"])]
    for l, (W, c) in enumerate(m["layers"]):
        out += [(f"W{l}", f"W{l}", W), (f"c{l}", f"c{l}", c)]
    return [x for x in out if x[2] is not None]


@pytest.mark.parametrize("case", tc.CASES, ids=[c["name"] for c in tc.CASES])
def test_tower_step_matches_the_float64_reference(case):
    rt = _rt()
    m = _tower_model(case)
    w, off = _extras(case)
    n = Net(m, case["relu_last"])
    opt = _dev_opt(rt, case["opt"])
    losses = n.net.step_full(opt, (m["ptr"], m["items"]), None, tuple(m["f"]), weights=w, item_offset=off, scale=2.0, l2_reg=0.01, l2_mlp=0.02,
                             chunk_items=case["chunk_items"], chunk_samples=case["chunk_samples"], labels=(m["lptr"], m["litems"]),
                             label_weights=m["lw"])
    e = tc.copy_model(m, np.float64)
    oo = tc.make_opt(case["opt"])
    want = lr.tower_step(e["H"], e["V"], e["b"], e["S"], e["layers"], m["ptr"], m["items"], m["f"], m["lptr"], m["litems"], oo, "mean",
                         case["relu_last"], _f64(m["lw"]), _f64(w), _f64(off), 2.0, float(np.float32(0.01)), float(np.float32(0.02)))
    _check_losses(case["name"], losses, want)
    for (name, key, W0), t, (_, _, w64) in zip(_named(m), n.tables(), _named(e)):
        got, w32 = t.read(), w64.astype(np.float32)
        print(f"{case['name']} {name}: rel err {rel_err(got, w32):.3g}")
        assert np.isfinite(got).all(), name
        if case["opt"] == "adam":
            assert rel_err(got, w32) <= TOL_ADAM, name
        else:
            delta_check(W0, got, w32, steps=1, what=f"{case['name']} {name}")


@pytest.mark.parametrize("si", range(len(tc.SHAPES)))
def test_tower_row_losses_are_within_the_bound_and_the_forward_is_the_steps_loss(si):
    rt = _rt()
    case = tc.shape_case(si)
    m = _tower_model(case)
    w, off = _extras(case, minus_inf=m["litems"])
    n = Net(m, case["relu_last"])
    before = [t.read().view(np.int32) for t in n.tables()]
    e = tc.copy_model(m, np.float64)
    q64 = tr.queries(e["H"], e["S"], e["layers"], m["ptr"], m["items"], m["f"], "mean", case["relu_last"])
    for lw in (m["lw"], None):
        kw = dict(weights=w, item_offset=off, scale=2.0, chunk_items=case["chunk_items"], labels=(m["lptr"], m["litems"]), label_weights=lw)
        fwd = n.net.loss_full((m["ptr"], m["items"]), None, tuple(m["f"]), per_row=True, **kw)
        want = lr.row_losses_q(q64, e["V"], e["b"], m["lptr"], m["litems"], _f64(lw), _f64(off), 2.0)
        bound = lr.row_bound_q(q64, e["V"], e["b"], m["lptr"], m["litems"], _f64(lw), off, 2.0)
        _check_rows(f"{case['name']} weights={lw is not None}", fwd[2], want, bound)
    assert _same(before, [t.read().view(np.int32) for t in n.tables()])
    losses = n.net.step_full(_dev_opt(rt, "sgd"), (m["ptr"], m["items"]), None, tuple(m["f"]), l2_reg=0.01, l2_mlp=0.02,
                             chunk_samples=case["chunk_samples"], **kw)
    assert _same_losses(fwd[:2], (losses[0][0], losses[1][0]))


def test_tower_train_masks_leave_every_other_table_bit_identical():
    rt = _rt()
    case = tc.CASES[0]
    m = _tower_model(case)
    for train in (("tower",), ("item", "bias"), ("history", "side")):
        n = Net(m, case["relu_last"])
        before = {name: t.read().view(np.int32) for (name, _, _), t in zip(_named(m), n.tables())}
        n.net.step_full(_dev_opt(rt, "adam"), (m["ptr"], m["items"]), None, tuple(m["f"]), l2_reg=0.01, l2_mlp=0.02, train=train,
                        labels=(m["lptr"], m["litems"]), label_weights=m["lw"])
        for (name, _, _), t in zip(_named(m), n.tables()):
            role = "tower" if name[0] in "Wc" else "side" if name.startswith("side") else name
            assert np.array_equal(before[name], t.read().view(np.int32)) == (role not in train), (train, name)


@pytest.mark.parametrize("D", [64, 50])
def test_an_identity_layer_is_seqrec_on_the_set_step_bit_for_bit(D):
    """no side tables, L = 1, W_0 = I, no bias, relu_last=False: x W is exact in fp32, so the tower is SeqRec -- row losses, loss,
    l2, and H, V and b after one SGD step"""
    rt = _rt()
    rng = np.random.default_rng(40 + D)
    case = dict(seed=41, B=130, NI=300)
    u = lambda *shape: rng.uniform(-fc.SCALE, fc.SCALE, shape).astype(np.float32)
    H, V, b = u(300, D), u(300, D), u(300, 1)
    ptr, items = fc.make_bags(case)
    lptr, litems, lw = lc.make_sets(case, weights=True)
    w = rng.uniform(0, 2, 130).astype(np.float32); off = rng.normal(0, 1, 300).astype(np.float32)
    deep = Net(dict(H=H, V=V, b=b, S=[], layers=[[np.eye(D, dtype=np.float32), None]]), relu_last=False)
    sH, sV, sb = _tables(rt, H, V, b)
    seq = rt.SeqRec(sH, sV, sb)
    kw = dict(weights=w, item_offset=off, chunk_items=128, labels=(lptr, litems), label_weights=lw)
    a = deep.net.loss_full((ptr, items), per_row=True, **kw)
    c = seq.loss_full((ptr, items), per_row=True, **kw)
    assert _same_losses(a[:2], c[:2]) and np.array_equal(a[2].view(np.int32), c[2].view(np.int32))
    la = deep.net.step_full(rt.Optimizer.sgd(0.05), (ptr, items), l2_reg=0.01, chunk_samples=64, train=("history", "item", "bias"), **kw)
    lc_ = seq.step_full(rt.Optimizer.sgd(0.05), (ptr, items), l2_reg=0.01, chunk_samples=64, **kw)
    assert _same_losses(la, lc_)
    for name, x, y, x0 in (("history", deep.H, sH, H), ("item", deep.V, sV, V), ("bias", deep.b, sb, b)):
        assert np.array_equal(x.read().view(np.int32), y.read().view(np.int32)), name
        assert not np.array_equal(x.read(), x0), name


# ---- the tf2 layer -------------------------------------------------------------------------------------------------------------------
def test_vanilla_youtube_rec_train_steps_sets_is_the_runtime_call():
    rt = _rt()
    from openrec_amd.tf2.recommenders import VanillaYouTubeRec
    case = dict(MID, D=32)
    H, V, b, ptr, items = lc.make_seq(case)
    lptr, litems, lw = lc.make_sets(case, weights=True)
    seq, lens = lc.padded(ptr, items, fill=0, extra=0)
    lab, lab_len = lc.padded(lptr, litems, fill=0)
    lwp = np.zeros(lab.shape, np.float32)
    lwp[np.arange(lab.shape[1])[None, :] < lab_len[:, None]] = lw
    w, off = _extras(case)
    L = seq.shape[1]
    model = VanillaYouTubeRec(32, L, case["NI"], l2_reg_embed=0.01)
    model.seq_item_latent_factor.table.write(H); model.item_latent_factor.table.write(V); model.item_bias.table.write(b)
    fwd = model.loss_sets(seq, lens, lab, lab_len, label_weight=lwp, sample_weight=w, item_offset=off)
    got = model.train_steps_sets(_dev_opt(rt, "adam"), seq, lens, lab, lab_len, label_weight=lwp, sample_weight=w, item_offset=off)
    tabs = _tables(rt, H, V, b)
    want = rt.SeqRec(*tabs, pool=("fixed", L)).step_full(_dev_opt(rt, "adam"), (ptr, items), weights=w, item_offset=off, l2_reg=0.01,
                                                         labels=(lptr, litems), label_weights=lw)
    assert _same_losses(got, want) and _same_losses(fwd, (got[0][0], got[1][0]))
    assert _same(_bits(model.seq_item_latent_factor.table, model.item_latent_factor.table, model.item_bias.table), _bits(*tabs))


def test_mult_dae_train_steps_is_the_runtime_call_and_serves_histories():
    rt = _rt()
    from openrec_amd.tf2.recommenders import MultDAE
    from openrec_amd.tf2.data import autoencoder_batches
    NI, D = 300, 32
    rng = np.random.default_rng(8)
    users = np.repeat(np.arange(90), rng.integers(1, 30, 90))
    raw = dict(user_id=users, item_id=rng.integers(0, NI, len(users)))
    bt = next(autoencoder_batches(raw, 90, 130, seed=2))
    model = MultDAE(D, NI, hidden=[24, 40], l2_reg_embed=0.01, l2_reg_mlp=0.02)
    T = lambda lf: lf.table.read()
    H, V, b = T(model.seq_item_latent_factor), T(model.item_latent_factor), T(model.item_bias)
    layers = [(T(W), T(c)) for W, c in zip(model.mlp_weights, model.mlp_biases)]
    assert V.shape == (NI, 40) and H.shape == (NI, D)
    got = model.train_steps(_dev_opt(rt, "adagrad"), bt["in_items"], bt["in_len"], bt["label_items"], bt["label_len"])
    tabs = _tables(rt, H, V, b)
    lt = [_tables(rt, W, c) for W, c in layers]
    ptr, items = rt.bags_to_ragged(bt["in_items"], bt["in_len"])
    lptr, litems = rt.bags_to_ragged(bt["label_items"], bt["label_len"])
    want = rt.DeepSeqRec(*tabs, lt, pool="mean").step_full(_dev_opt(rt, "adagrad"), (ptr, items), l2_reg=0.01, l2_mlp=0.02, labels=(lptr, litems))
    assert _same_losses(got, want) and np.isfinite(got[0]).all()
    mine = [model.seq_item_latent_factor, model.item_latent_factor, model.item_bias] + [x for p in zip(model.mlp_weights, model.mlp_biases) for x in p]
    assert _same(_bits(*[lf.table for lf in mine]), _bits(*tabs, *[t for p in lt for t in p]))
    ids, scores = model.recommend(bt["in_items"][:7], bt["in_len"][:7], 5)
    assert ids.shape == (7, 5) and np.isfinite(np.asarray(scores)).all()
