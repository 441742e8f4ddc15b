"""GPU: the graph propagation (`rt.graph_spmm`, `rt.LightGCN.propagate`), the dense optimizer apply and the LightGCN train step
against the float64 references of tests/lightgcn_ref.py.  The exact cases are bit equality with float64 (every term and partial
sum is representable: a dropped, doubled or mis-weighted entry is a bit difference); the general graphs are held to the
worst-case bound L (n_max + 8) u P(|U|, |V|) that tests/test_lightgcn_cpu.py validates; the step goes through
conftest.delta_check / TOL_ADAM."""
import numpy as np
import pytest

import conftest as cf
import lightgcn_cases as lc
import lightgcn_ref as lr

pytestmark = pytest.mark.gpu


def _rt():
    from openrec_amd import runtime as rt
    return rt


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _graph(rt, by_user, by_item, norm):
    nu, ni = by_user[0].size - 1, by_item[0].size - 1
    return rt.InteractionGraph(lr.records_of(*by_user), nu, ni, norm=norm)


def _model(rt, U, V, by_user, by_item, norm, L, weights=None):
    tu = rt.Table(*U.shape).write(U); tv = rt.Table(*V.shape).write(V)
    return rt.LightGCN(tu, tv, _graph(rt, by_user, by_item, norm), layers=L, layer_weights=weights), tu, tv


def _propagated(rt, U, V, by_user, by_item, norm, L, weights=None):
    net, tu, tv = _model(rt, U, V, by_user, by_item, norm, L, weights)
    Uf, Vf = net.propagate()
    out = Uf.read(), Vf.read()
    assert np.array_equal(_bits(tu.read()), _bits(U)) and np.array_equal(_bits(tv.read()), _bits(V)), "propagate changed a layer-0 table"
    return out


# ------------------------------------------------------------------------------------------------- exact cases ---
def test_long_rows_are_exact():
    rt = _rt()
    S = rt.graph_segment_len()
    by_user, by_item = lc.long_graph(S)
    U, V = lc.int_tables(lc.LONG_NU, lc.LONG_NI, 16, 1)
    al = np.ones(3, np.float32)
    fu, fv = lr.propagate(U, V, by_user, by_item, lr.unit(lc.LONG_NU), lr.unit(lc.LONG_NI), al)
    gu, gv = _propagated(rt, U, V, by_user, by_item, "none", 2, (1, 1, 1))
    assert np.array_equal(gu.astype(np.float64), fu) and np.array_equal(gv.astype(np.float64), fv)


@pytest.mark.parametrize("D", (16, 50))
def test_symmetric_weights_are_exact_on_a_biregular_graph(D):
    rt = _rt()
    by_user, by_item = lc.biregular()
    U, V = lc.int_tables(64, 16, D, 20 + D)
    fu, fv = lr.propagate(U, V, by_user, by_item, lr.scales(by_user[0]), lr.scales(by_item[0]), lc.default_weights(3))
    gu, gv = _propagated(rt, U, V, by_user, by_item, "sym", 3)
    assert np.array_equal(gu.astype(np.float64), fu) and np.array_equal(gv.astype(np.float64), fv)


@pytest.mark.parametrize("D", (1, 50, 64, 100, 128))
def test_every_dim_is_exact_on_the_long_rows(D):
    rt = _rt()
    by_user, by_item = lc.long_graph(rt.graph_segment_len())
    U, V = lc.int_tables(lc.LONG_NU, lc.LONG_NI, D, 10 + D)
    fu, fv = lr.propagate(U, V, by_user, by_item, lr.unit(lc.LONG_NU), lr.unit(lc.LONG_NI), np.ones(2, np.float32))
    gu, gv = _propagated(rt, U, V, by_user, by_item, "none", 1, (1, 1))
    assert np.array_equal(gu.astype(np.float64), fu) and np.array_equal(gv.astype(np.float64), fv)


# -------------------------------------------------------------------------------------------------- invariance ---
def _spmm(rt, X, csr, n_out, rows=None, rs=None, cs=None, acc0=None, alpha=0.0, out0=None):
    tx = rt.Table(*X.shape).write(X)
    out = rt.Table(n_out, X.shape[1]).write(out0 if out0 is not None else np.full((n_out, X.shape[1]), 7.0, np.float32))
    acc = rt.Table(n_out, X.shape[1]).write(acc0) if acc0 is not None else None
    for r in (rows if isinstance(rows, list) else [rows]):
        rt.graph_spmm(tx, out, csr, row_scale=rs, col_scale=cs, rows=r, acc=acc, acc_alpha=alpha)
    return out.read(), (acc.read() if acc is not None else None)


@pytest.mark.parametrize("D", (64, 50))
def test_a_row_is_a_function_of_its_own_data(D):
    """items <- users on the long-row graph with float tables and scales: one call == three calls cut at 1, 7, end == host CSR
    == device CSR, bit for bit; rows outside a range are not written"""
    rt = _rt()
    by_user, by_item = lc.long_graph(rt.graph_segment_len())
    U, _ = lc.float_tables(lc.LONG_NU, lc.LONG_NI, D, 31)
    rs, cs = lr.scales(by_item[0]), lr.scales(by_user[0])
    host = rt.ALSCsr(by_item[0], by_item[1], None, lc.LONG_NU)
    dev = host.to_device()
    acc0 = np.full((lc.LONG_NI, D), 0.25, np.float32)
    one, acc_one = _spmm(rt, U, host, lc.LONG_NI, rs=rs, cs=cs, acc0=acc0, alpha=0.5)
    ref = lr.half_layer(U, *by_item, rs, cs)
    assert np.abs(one - ref).max() <= 1e-5 * np.abs(ref).max()
    assert np.array_equal(_bits(one[0]), np.zeros(D, np.int32)), "the empty row is not all +0.0"
    assert np.array_equal(_bits(acc_one[0]), _bits(acc0[0])), "acc of the empty row changed"
    assert np.array_equal(_bits(acc_one[1:]), _bits(acc0[1:] + np.float32(0.5) * one[1:]))
    three, acc_three = _spmm(rt, U, host, lc.LONG_NI, rows=[(0, 1), (1, 6), range(7, lc.LONG_NI)], rs=rs, cs=cs, acc0=acc0, alpha=0.5)
    on_dev, acc_dev = _spmm(rt, U, dev, lc.LONG_NI, rs=rs, cs=cs, acc0=acc0, alpha=0.5)
    dev_three, _ = _spmm(rt, U, dev, lc.LONG_NI, rows=[(0, 1), (1, 6), (7, lc.LONG_NI - 7)], rs=rs, cs=cs)
    for other in (three, on_dev, dev_three):
        assert np.array_equal(_bits(other), _bits(one))
    assert np.array_equal(_bits(acc_three), _bits(acc_one)) and np.array_equal(_bits(acc_dev), _bits(acc_one))
    part, _ = _spmm(rt, U, dev, lc.LONG_NI, rows=(8, 2), rs=rs, cs=cs)
    assert np.array_equal(_bits(part[8:10]), _bits(one[8:10])) and (np.delete(part, (8, 9), axis=0) == 7.0).all()
    none, _ = _spmm(rt, U, dev, lc.LONG_NI, rows=(3, 0), rs=rs, cs=cs)
    assert (none == 7.0).all(), "nrows == 0 wrote something"


@pytest.mark.parametrize("D", (64, 50))
@pytest.mark.parametrize("slots", (0, 3, 7, 11))
def test_rows_without_a_scratch_slot_walk_their_segments_to_the_same_bits(D, slots):
    """a device CSR with fewer scratch slots than the long rows have segments (the long-row graph needs 2 + 2 + 3 + 3 + 5 + 10 =
    25): 0 -- no plan at all, every long row walks alone; 3, 7, 11 -- the plan hands out what there is, rows that ask for more
    than is left get none, and whatever of the slot list nobody owns is skipped by the segment launch"""
    rt = _rt()
    S = rt.graph_segment_len()
    by_user, by_item = lc.long_graph(S)
    need = sum((n + S - 1) // S for n in lc.long_degrees(S) if n > S)
    U, _ = lc.float_tables(lc.LONG_NU, lc.LONG_NI, D, 31)
    rs, cs = lr.scales(by_item[0]), lr.scales(by_user[0])
    dev = rt.ALSCsr(by_item[0], by_item[1], None, lc.LONG_NU).to_device()
    assert rt.graph_long_segments(dev) == need and slots < need
    full, _ = _spmm(rt, U, dev, lc.LONG_NI, rs=rs, cs=cs)
    tx = rt.Table(*U.shape).write(U); out = rt.Table(lc.LONG_NI, D).fill(7.0)
    rt.graph_spmm(tx, out, dev, row_scale=rs, col_scale=cs, long_segments=slots)
    assert np.array_equal(_bits(out.read()), _bits(full))


def test_non_finite_inputs_give_non_finite_outputs():
    rt = _rt()
    by_user, by_item = lc.biregular()
    U, _ = lc.int_tables(64, 16, 16, 3)
    U[5, 2] = np.nan; U[9, 0] = np.inf
    out, _ = _spmm(rt, U, rt.ALSCsr(by_item[0], by_item[1], None, 64), 16)
    assert not np.isfinite(out).all() and np.isfinite(out[:, 1]).all()


# ------------------------------------------------------------------------------------------------ general graphs ---
@pytest.mark.parametrize("D,L", lc.GEN_CASES)
def test_general_graph_within_the_worst_case_bound(D, L):
    rt = _rt()
    h = lc.general_case(D, L)
    gu, gv = _propagated(rt, h["U"], h["V"], h["by_user"], h["by_item"], "sym", L)
    for got, ref, bd, e0 in ((gu, h["fu"], h["bu"], h["U"]), (gv, h["fv"], h["bv"], h["V"])):
        err = np.abs(got.astype(np.float64) - ref)
        print(f"D {D} L {L}: max err / max|ref| {err.max() / np.abs(ref).max():.3g}")
        assert np.isfinite(got).all() and (err <= bd).all(), float((err / np.maximum(bd, 1e-300)).max())
    # rows with no path: alpha_0 E(0) exactly
    a0 = h["al"][0]
    assert np.array_equal(_bits(gu[lc.GEN_EMPTY_USER]), _bits(a0 * h["U"][lc.GEN_EMPTY_USER]))
    empty = np.diff(h["by_item"][0]) == 0
    assert np.array_equal(_bits(gv[empty]), _bits(a0 * h["V"][empty]))


# ------------------------------------------------------------------------------------------------------ the step ---
def _hold_losses(what, losses, ref_losses, l2_reg):
    """the returned loss and l2 of every graph step within conftest.TOL relative of float64, whatever the optimizer"""
    assert len(losses) == len(ref_losses)
    for k, ((loss, l2), (rl, rl2)) in enumerate(zip(losses, ref_losses)):
        print(f"{what} step {k}: loss rel {abs(loss - rl) / abs(rl):.3g}, l2 rel {abs(l2 - rl2) / max(abs(rl2), 1e-30):.3g}")
        assert abs(loss - rl) <= cf.TOL * abs(rl) and abs(l2 - rl2) <= cf.TOL * max(abs(rl2), 1e-30), (what, k, loss, rl, l2, rl2)
        assert (l2 == 0.0) == (l2_reg == 0.0)


def _native_opt(rt, name):
    kind, kw = lc.OPTS[name][1]
    return getattr(rt.Optimizer, kind)(**kw)


def _run_steps(rt, opt_name, steps, l2_reg, train=None, mixed=False):
    s = lc.step_setup()
    net, tu, tv = _model(rt, s["U"], s["V"], s["by_user"], s["by_item"], "sym", lc.STEP_L)
    opt = _native_opt(rt, opt_name)
    bs = lc.step_batches()
    losses = []
    if mixed:
        losses.append(net.step(opt, *bs[0], l2_reg=l2_reg))
        rt.pairwise_step("bpr", opt, tu, tv, None, *bs[1], no_l2=True)
        losses.append(net.step(opt, *bs[2], l2_reg=l2_reg))
    else:
        for k in range(steps):
            losses.append(net.step(opt, *bs[k], l2_reg=l2_reg, train=train))
    return tu.read(), tv.read(), losses, (net, opt, tu, tv)


@pytest.mark.parametrize("l2_reg", (0.0, 0.01))
@pytest.mark.parametrize("steps", (1, 3))
@pytest.mark.parametrize("opt", ("sgd", "momentum", "nesterov", "adagrad"))
def test_step_against_float64(opt, steps, l2_reg):
    rt = _rt()
    s = lc.step_setup()
    U64, V64, ref_losses = lc.step_ref(opt, steps, l2_reg)
    gu, gv, losses, _ = _run_steps(rt, opt, steps, l2_reg)
    for what, w0, got, want in (("U", s["U"], gu, U64), ("V", s["V"], gv, V64)):
        coef = cf.delta_check(w0, got, want.astype(np.float32), steps=steps, what=f"{opt} {what}")
        print(f"{opt} x{steps} l2 {l2_reg} {what}: projection {coef:.6f}, max|d| {np.abs(want - w0).max():.3g}")
        assert abs(coef - 1.0) <= 1e-3
    _hold_losses(f"{opt} x{steps}", losses, ref_losses, l2_reg)
    if opt == "sgd":           # no path to the batch, no occurrence in it: zero gradient, bit-unchanged
        assert np.array_equal(_bits(gu[lc.GEN_EMPTY_USER]), _bits(s["U"][lc.GEN_EMPTY_USER]))
        assert np.array_equal(_bits(gv[-10:]), _bits(s["V"][-10:]))


@pytest.mark.parametrize("l2_reg", (0.0, 0.01))
def test_adam_step_against_float64(l2_reg):
    rt = _rt()
    U64, V64, ref_losses = lc.step_ref("adam", 3, l2_reg)
    gu, gv, losses, _ = _run_steps(rt, "adam", 3, l2_reg)
    print("adam rel_err", cf.rel_err(gu, U64), cf.rel_err(gv, V64))
    assert cf.rel_err(gu, U64) <= cf.TOL_ADAM and cf.rel_err(gv, V64) <= cf.TOL_ADAM
    _hold_losses("adam x3", losses, ref_losses, l2_reg)


@pytest.mark.parametrize("opt", ("adam", "momentum"))
def test_rows_without_a_gradient_follow_the_dense_rule(opt):
    """the empty user and the empty items under Adam / momentum: the dense rule with zero gradient (nothing moves: m = v = 0),
    and rows of the graph far from the batch move exactly as the float64 rule says"""
    rt = _rt()
    s = lc.step_setup()
    U64, V64, _ = lc.step_ref(opt, 3, 0.0)
    gu, gv, _, _ = _run_steps(rt, opt, 3, 0.0)
    assert np.array_equal(U64[lc.GEN_EMPTY_USER], s["U"][lc.GEN_EMPTY_USER].astype(np.float64))
    assert np.array_equal(_bits(gu[lc.GEN_EMPTY_USER]), _bits(s["U"][lc.GEN_EMPTY_USER]))
    assert np.array_equal(_bits(gv[-10:]), _bits(s["V"][-10:]))
    tol = cf.TOL_ADAM if opt == "adam" else cf.TOL
    assert cf.rel_err(gu[40:], U64[40:]) <= tol, "users outside every batch (gradient through the graph only)"


def test_train_user_only_leaves_the_items_bit_identical():
    rt = _rt()
    s = lc.step_setup()
    U64, V64, _ = lc.step_ref("sgd", 1, 0.01, train_tables=("user",))
    gu, gv, _, _ = _run_steps(rt, "sgd", 1, 0.01, train=("user",))
    assert np.array_equal(_bits(gv), _bits(s["V"]))
    assert abs(cf.delta_check(s["U"], gu, U64.astype(np.float32), steps=1, what="user only") - 1.0) <= 1e-3
    gu2, gv2, _, _ = _run_steps(rt, "sgd", 1, 0.01, train=("item",))
    assert np.array_equal(_bits(gu2), _bits(s["U"])) and not np.array_equal(_bits(gv2), _bits(s["V"]))


@pytest.mark.parametrize("opt", ("sgd", "adam"))
def test_two_runs_of_a_step_give_the_same_bits(opt):
    rt = _rt()
    a = _run_steps(rt, opt, 2, 0.01)
    b = _run_steps(rt, opt, 2, 0.01)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    assert not np.array_equal(_bits(a[0]), _bits(lc.step_setup()["U"]))


def test_graph_steps_and_pairwise_steps_share_tables_and_adam():
    rt = _rt()
    U64, V64, ref_losses = lc.step_ref("adam", 3, 0.01, mixed=True)
    gu, gv, losses, (net, opt, tu, tv) = _run_steps(rt, "adam", 3, 0.01, mixed=True)
    print("mixed rel_err", cf.rel_err(gu, U64), cf.rel_err(gv, V64))
    assert opt.step == 3
    assert cf.rel_err(gu, U64) <= cf.TOL_ADAM and cf.rel_err(gv, V64) <= cf.TOL_ADAM
    _hold_losses("graph, bpr, graph", losses, ref_losses, 0.01)


def test_loss_is_the_forward_alone():
    rt = _rt()
    s = lc.step_setup()
    net, tu, tv = _model(rt, s["U"], s["V"], s["by_user"], s["by_item"], "sym", lc.STEP_L)
    uid, pid, nid = lc.step_batches()[0]
    rl, rl2, _, _ = lr.loss_dense(s["A"], s["U"], s["V"], s["al"], uid, pid, nid, 0.01)
    loss, l2 = net.loss(uid, pid, nid, l2_reg=0.01)
    assert abs(loss - rl) <= cf.TOL * abs(rl) and abs(l2 - rl2) <= cf.TOL * abs(rl2)
    assert np.array_equal(_bits(tu.read()), _bits(s["U"])) and np.array_equal(_bits(tv.read()), _bits(s["V"]))
    import torch
    dv = [torch.from_numpy(x).cuda() for x in (uid, pid, nid)]
    dloss, dl2 = net.loss(*dv, l2_reg=0.01)              # ids already on the device
    assert abs(dloss - loss) <= cf.TOL * abs(loss) and abs(dl2 - l2) <= cf.TOL * abs(l2)


def test_table_apply_dense_is_the_dense_rule():
    rt = _rt()
    import torch
    rng = np.random.default_rng(5)
    W = rng.uniform(-0.5, 0.5, (37, 50)).astype(np.float32)
    G = [rng.uniform(-0.1, 0.1, W.shape).astype(np.float32) for _ in range(2)]
    for name in ("sgd", "momentum", "nesterov", "adagrad", "adam"):
        t = rt.Table(*W.shape).write(W)
        opt = _native_opt(rt, name)
        ref, w64 = lr.DenseOpt(**lc.OPTS[name][0]), W.astype(np.float64)
        for g in G:
            rt.table_apply_dense(opt, t, torch.from_numpy(g).cuda())
            ref.advance(); w64 = ref.apply("w", w64, g.astype(np.float64))
        assert cf.rel_err(t.read(), w64) <= (cf.TOL_ADAM if name == "adam" else cf.TOL), name
        if name == "adam":
            assert opt.step == 2


# ------------------------------------------------------------------------------------------------------- surface ---
def test_recommend_topk_on_the_propagated_tables():
    rt = _rt()
    h = lc.topk_case()
    net, _, _ = _model(rt, h["U"], h["V"], h["by_user"], h["by_item"], "sym", lc.TOPK["L"])
    Uf, Vf = net.propagate()
    items, scores = rt.recommend_topk("dot", Uf, Vf, None, h["users"], lc.TOPK["k"])
    for got, want in zip(np.asarray(items), h["items"]):
        assert set(got.tolist()) == set(want.tolist())


def test_tf2_wrapper():
    rt = _rt()
    from openrec_amd.tf2.recommenders import LightGCN
    s = lc.step_setup()
    bs = lc.step_batches()
    model = LightGCN(lc.STEP_D, lc.GEN_NU, lc.GEN_NI, layers=lc.STEP_L, l2_reg=0.01)
    model.user_latent_factor.table.write(s["U"]); model.item_latent_factor.table.write(s["V"])
    model.fit_graph(lr.records_of(*s["by_user"]))
    users = np.arange(0, 40, dtype=np.int32)
    before, _ = model.recommend(users, 5)
    opt = _native_opt(rt, "sgd")
    ids = [np.stack([b[j] for b in bs[:2]]) for j in range(3)]
    loss, l2 = model.train_steps(opt, *ids)
    gu, gv, losses, _ = _run_steps(rt, "sgd", 2, 0.01)
    assert np.array_equal(_bits(model.user_latent_factor.table.read()), _bits(gu))
    assert np.array_equal(_bits(model.item_latent_factor.table.read()), _bits(gv))
    assert loss.shape == (2,) and abs(loss[0] - losses[0][0]) <= cf.TOL * abs(losses[0][0])
    # recommend after the steps sees the new tables: the propagation of what the tables hold now
    Uf, Vf = model.propagated()
    fu, fv = lr.propagate(gu, gv, s["by_user"], s["by_item"], s["su"], s["sv"], s["al"])
    assert cf.rel_err(Uf.read(), fu) <= cf.TOL and cf.rel_err(Vf.read(), fv) <= cf.TOL
    items, scores = model.recommend(users, 5)
    want = np.take_along_axis(Uf.read()[users] @ Vf.read().T, np.asarray(items), axis=1)
    assert np.abs(np.asarray(scores) - want).max() <= 1e-5 * np.abs(want).max()
    assert np.asarray(model.inference(users)).shape == (40, lc.GEN_NI)


@pytest.mark.parametrize("name", ("sgd", "momentum", "adagrad", "adam"))
def test_tf2_wrapper_takes_the_keras_optimizers(name):
    """tf.keras.optimizers.{SGD, Adagrad, Adam} through the shim give the bits of the native optimizer of the same settings"""
    rt = _rt()
    from openrec_amd.tf2.compat import optimizers
    from openrec_amd.tf2.recommenders import LightGCN
    s = lc.step_setup()
    bs = lc.step_batches()
    kw = dict(lc.OPTS[name][1][1]); lr_ = kw.pop("lr")
    keras = {"sgd": optimizers.SGD, "momentum": optimizers.SGD, "adagrad": optimizers.Adagrad, "adam": optimizers.Adam}[name](learning_rate=lr_, **kw)
    model = LightGCN(lc.STEP_D, lc.GEN_NU, lc.GEN_NI, layers=lc.STEP_L, l2_reg=0.01)
    model.user_latent_factor.table.write(s["U"]); model.item_latent_factor.table.write(s["V"])
    model.fit_graph(lr.records_of(*s["by_user"]))
    ids = [np.stack([b[j] for b in bs[:2]]) for j in range(3)]
    model.train_steps(keras, *ids)
    gu, gv, _, _ = _run_steps(rt, name, 2, 0.01)
    assert np.array_equal(_bits(model.user_latent_factor.table.read()), _bits(gu))
    assert np.array_equal(_bits(model.item_latent_factor.table.read()), _bits(gv))


def test_tf2_wrapper_scores_and_evaluates_on_the_propagated_tables():
    rt = _rt()
    from openrec_amd.tf2.recommenders import LightGCN
    s = lc.step_setup()
    model = LightGCN(lc.STEP_D, lc.GEN_NU, lc.GEN_NI, layers=lc.STEP_L, l2_reg=0.01)
    model.user_latent_factor.table.write(s["U"]); model.item_latent_factor.table.write(s["V"])
    model.fit_graph(lr.records_of(*s["by_user"]))
    model.train_steps(rt.Optimizer.sgd(lr=1.0), *lc.step_batches()[0])
    Uf, Vf = model.propagated()
    ptr, cols = s["by_user"]
    users = np.array([u for u in range(40) if ptr[u + 1] - ptr[u] >= 4][:24], np.int32)
    full = np.asarray(model.inference(users))
    cand = [np.array([3, 199, 0, 3, 57 + int(u)], np.int32) for u in users]
    for u, (sc, c) in enumerate(zip(model.score(users, cand), cand)):
        assert np.array_equal(_bits(sc), _bits(full[u, c])), "score differs from inference at the same places"
    assert np.abs(full - Uf.read()[users] @ Vf.read().T).max() <= 1e-5 * np.abs(full).max()
    # evaluate: the metrics of the propagated tables through the path every recommender uses
    pos = rt.SparseMask.from_lists([cols[ptr[u]:ptr[u + 1]][:2] for u in users], lc.GEN_NI)
    excl = rt.SparseMask.from_lists([cols[ptr[u]:ptr[u + 1]][2:] for u in users], lc.GEN_NI)
    got = model.evaluate(users, pos, excl, at=(10,), score_matrix=False)
    want = rt.rank_metrics_matrixfree(pos, excl, [10], kind="dot", user=Uf, item=Vf, bias=None, uid=users)
    assert set(got) == set(want) == {"auc", "ndcg", "recall"}
    for k in want:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
    raw = rt.rank_metrics_matrixfree(pos, excl, [10], kind="dot", user=model.user_latent_factor.table, item=model.item_latent_factor.table,
                                     bias=None, uid=users)
    assert not all(np.array_equal(np.asarray(got[k]), np.asarray(raw[k])) for k in raw), "evaluate ran on the raw tables"


# ------------------------------------------------------------------------------------------------ argument errors ---
def test_library_refuses_bad_arguments_with_the_tables_untouched():
    rt = _rt()
    from openrec_amd import _ffi
    by_user, by_item = lc.biregular()
    U, V = lc.int_tables(64, 16, 16, 3)
    tu = rt.Table(*U.shape).write(U); tv = rt.Table(*V.shape).write(V); tv2 = rt.Table(*V.shape).write(V)
    t8 = rt.Table(16, 8).write(np.zeros((16, 8), np.float32))
    other = rt.Table(16, 16, ctx=rt.Context(0)).write(V)
    lib, c = tu.ctx._lib, tu.ctx._h
    csr = rt.ALSCsr(by_item[0], by_item[1], None, 64)
    p, cl = csr.ptr.ctypes.data, csr.cols.ctypes.data

    def call(X, out, acc, row0=0, nrows=16, flags=0):
        return lib.orx_graph_spmm(c, X._h, out._h, acc._h if acc is not None else None, 1.0, p, cl, None, None, row0, nrows, -1, flags)
    assert call(tu, tv, None) == _ffi.ORX_OK
    for bad in (call(tv, tv, None), call(tv, tv2, tv), call(tu, t8, None), call(tu, tv, None, row0=10, nrows=7), call(tu, tv, None, row0=-1),
                call(tu, other, None), call(tu, tv, other), call(tu, tv, None, flags=64)):
        assert bad == _ffi.ORX_ERR_ARG
    assert np.array_equal(_bits(tu.read()), _bits(U)) and np.array_equal(_bits(tv2.read()), _bits(V))
    g = _graph(rt, by_user, by_item, "sym")
    for kw in (dict(layers=0), dict(layers=9), dict(layers=2, layer_weights=(1, 1))):
        with pytest.raises(ValueError):
            rt.LightGCN(tu, tv2, g, **kw)
    with pytest.raises(ValueError):
        rt.LightGCN(tu, rt.Table(17, 16), g)
    with pytest.raises(ValueError):
        rt.LightGCN(tu, other, g)
    net = rt.LightGCN(tu, tv2, g, layers=2)
    ids = (np.zeros(4, np.int32),) * 3
    with pytest.raises(ValueError):
        net.step(rt.Optimizer.sgd(lr=0.1), *ids, l2_reg=-1.0)
    with pytest.raises(ValueError):
        net.step(rt.Optimizer.sgd(lr=0.1), *ids, train=("bias",))
    assert np.array_equal(_bits(tu.read()), _bits(U)) and np.array_equal(_bits(tv2.read()), _bits(V))


def test_a_column_outside_the_table_raises_index_error():
    rt = _rt()
    by_user, by_item = lc.biregular()
    U, _ = lc.int_tables(64, 16, 16, 3)
    cols = by_item[1].copy(); cols[5] = 64
    bad = rt.ALSCsr(by_item[0], cols, None, 64)
    with pytest.raises(IndexError):
        _spmm(rt, U, bad, 16)
    with pytest.raises(IndexError):
        _spmm(rt, U, bad.to_device(), 16)
    good, _ = _spmm(rt, U, rt.ALSCsr(by_item[0], by_item[1], None, 64), 16)      # the context stays usable
    assert np.isfinite(good).all()
