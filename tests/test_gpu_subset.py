"""Train steps over a SUBSET of a model's tables (`rt.pairwise_step(..., train=...)`, `rt.pointwise_step(..., train=...)`,
`apply_gradients` on a shorter variable list, `LatentFactor.trainable = False`): the trained tables and their slots against
an expectation composed from the oracle's own pieces -- gradients on the pre-step tables, `opt.begin_step()`, then
`opt.apply` for the trained roles only --, the frozen tables and their slots bit-for-bit against their values before the call.
Tolerances are the project's: conftest.delta_check / TOL for SGD, Adagrad and momentum, TOL_ADAM for Adam."""
import itertools

import numpy as np
import pytest

from conftest import TOL, TOL_ADAM, delta_check, rel_err
from subset_expect import Momentum, expect_step as _expect_step

pytestmark = pytest.mark.gpu

NU, NI, B, K = 300, 400, 512, 3
ROLES = ("user", "item", "bias")
STRICT = [c for r in (1, 2) for c in itertools.combinations(ROLES, r)]
STRICT_NB = [("user",), ("item",)]
OPTS = ("sgd", "adagrad", "adam", "momentum")
LR = {"sgd": 0.05, "adagrad": 0.05, "adam": 0.002, "momentum": 0.05}
KEY = {"user": "U", "item": "V", "bias": "b"}


def _rt():
    from openrec_amd import runtime as rt
    return rt


def _opts(name, rt):
    """(device optimizer, oracle optimizer)"""
    from oracle import numpy_oracle as orc
    lr = LR[name]
    if name == "sgd":
        return rt.Optimizer.sgd(lr), orc.SGD(lr)
    if name == "adagrad":
        return rt.Optimizer.adagrad(lr), orc.Adagrad(lr)
    if name == "adam":
        return rt.Optimizer.adam(lr), orc.AdamTFSparse(lr)
    return rt.Optimizer.momentum(lr, 0.9, True), Momentum(lr, 0.9, True)


def _slots(oo, key):
    """the oracle optimizer's slots of a variable, in the device's slot order"""
    if oo.kind == "adagrad":
        return [oo.acc[key]]
    if oo.kind == "adam":
        return [oo.m[key], oo.v[key]]
    if oo.kind == "momentum":
        return [oo.vel[key]]
    return []


def _case(seed, D, pointwise=False):
    rng = np.random.default_rng(seed)
    U = rng.uniform(-.05, .05, (NU, D)).astype(np.float32)
    V = rng.uniform(-.05, .05, (NI, D)).astype(np.float32)
    b = rng.uniform(-.05, .05, (NI, 1)).astype(np.float32)
    uid = rng.integers(0, NU, (K, B)).astype(np.int32)
    pid = rng.integers(0, NI, (K, B)).astype(np.int32)
    nid = rng.integers(0, NI, (K, B)).astype(np.int32)
    lab = (rng.random((K, B)) < 0.3).astype(np.float32)
    # the duplicates the semantics are about (512 ids over 300 users / 400 items: they hold by counting; kept as assertions)
    for s in range(K):
        assert np.unique(uid[s]).size < B, "some user must occur twice in a step"
        if pointwise:
            assert np.unique(pid[s]).size < B, "some item must occur twice in a step"
        else:
            assert np.intersect1d(pid[s], nid[s]).size > 0, "some item must occur as a positive and as a negative in a step"
    return U, V, b, uid, pid, nid, lab


def _device_step(rt, model, opt, tU, tV, tb, ids, k, train, **kw):
    if model == "wrmf":
        return rt.pointwise_step("wrmf", opt, tU, tV, tb, None, ids[0], ids[1], ids[2], K=k, B=B, a=2.0, b_w=0.5, train=train, **kw)
    return rt.pairwise_step(model, opt, tU, tV, tb, ids[0], ids[1], ids[2], K=k, B=B, margin=0.5, train=train, **kw)


def _ids_of(model, uid, pid, nid, lab, s=None):
    third = lab if model == "wrmf" else nid
    if s is None:
        return uid, pid, third
    return uid[s], pid[s], third[s]


NSLOT = {"sgd": 0, "adagrad": 1, "adam": 2, "momentum": 1}


def _run_and_check(model, optname, D, roles, has_bias=True, split=False, device_ids=False, seed=0, warm_up=True):
    """One full step first (device and oracle alike), so that every table has its optimizer slots and, under Adam, is lazily
    applied when the subset steps begin; then K steps over `roles`.  Trained tables and slots against the composed expectation;
    every frozen table and every slot of it bit-for-bit against its value before the subset call."""
    rt = _rt()
    U, V, b, uid, pid, nid, lab = _case(seed + D, D, pointwise=model == "wrmf")
    rng = np.random.default_rng(1000 + seed)
    warm = (rng.integers(0, NU, B).astype(np.int32), rng.integers(0, NI, B).astype(np.int32),
            (rng.random(B) < 0.3).astype(np.float32) if model == "wrmf" else rng.integers(0, NI, B).astype(np.int32))
    bz = b if has_bias else np.zeros_like(b)
    tU = rt.Table(NU, D).write(U); tV = rt.Table(NI, D).write(V); tb = rt.Table(NI, 1).write(b) if has_bias else None
    tabs = {"user": tU, "item": tV, "bias": tb}
    host = {"user": U, "item": V, "bias": bz}
    orig = {r: w.copy() for r, w in host.items()}
    opt, oo = _opts(optname, rt)
    if warm_up:
        _device_step(rt, model, opt, tU, tV, tb, warm, 1, None)
        _expect_step(model, U, V, bz, warm, oo, ROLES if has_bias else ("user", "item"))
    nslot = NSLOT[optname] if warm_up else 0        # (without the full step a frozen table has no slots)
    frozen = [r for r in ROLES if r not in roles and tabs[r] is not None]
    before = {r: [tabs[r].read()] + [opt.slot(tabs[r], k) for k in range(nslot)] for r in frozen}
    start = {r: tabs[r].read() for r in ROLES if tabs[r] is not None}
    ids = _ids_of(model, uid, pid, nid, lab)
    if device_ids:
        import torch
        ids = tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in ids)
    if split:
        out = [_device_step(rt, model, opt, tU, tV, tb, tuple(x[s] for x in ids), 1, roles) for s in range(K)]
        loss = np.array([o[0][0] for o in out]); l2 = np.array([o[1][0] for o in out])
    else:
        loss, l2 = _device_step(rt, model, opt, tU, tV, tb, ids, K, roles)
    for s in range(K):
        lw, l2w = _expect_step(model, U, V, bz, _ids_of(model, uid, pid, nid, lab, s), oo, roles)
        print(f"{model} {optname} D={D} {roles} step {s}: loss {loss[s]:.8g} want {lw:.8g}  l2 {l2[s]:.8g} want {l2w:.8g}")
        assert abs(loss[s] - lw) <= TOL * abs(lw) and abs(l2[s] - l2w) <= TOL * abs(l2w), (s, loss[s], lw, l2[s], l2w)
    what = f"{model} {optname} D={D} train={roles}"
    for r in frozen:
        after = [tabs[r].read()] + [opt.slot(tabs[r], k) for k in range(nslot)]
        for k, (x, y) in enumerate(zip(before[r], after)):
            assert np.array_equal(x, y), f"{what}: frozen {r} " + ("table" if k == 0 else f"slot {k - 1}") + " moved"
    for r in roles:
        t = tabs[r]
        got = t.read()
        print(f"{what} {r}: rel err {rel_err(got, host[r]):.3g}")
        if optname == "adam":
            assert rel_err(got, host[r]) <= TOL_ADAM, (what, r)
        else:
            delta_check(orig[r], got, host[r], steps=K + 1, what=f"{what} {r}")      # (the warm-up step and the K steps, from the first start)
        for k, want in enumerate(_slots(oo, KEY[r])):
            e = rel_err(opt.slot(t, k), want)
            print(f"{what} {r} slot {k}: rel err {e:.3g}")
            assert e <= (TOL_ADAM if optname == "adam" else TOL), (what, r, k, e)      # (Adam, tables and slots alike: TOL_ADAM)
    return tabs, opt, start


PAIR_CASES = [(m, o, D, r) for m in ("bpr", "ucml") for o in OPTS for D in (50, 64) for r in STRICT]


@pytest.mark.parametrize("model,optname,D,roles", PAIR_CASES)
def test_pairwise_subset_matches_the_composed_expectation(model, optname, D, roles):
    _run_and_check(model, optname, D, roles)


@pytest.mark.parametrize("optname,D,roles", [(o, D, r) for o in OPTS for D in (50, 64) for r in STRICT])
def test_wrmf_subset_matches_the_composed_expectation(optname, D, roles):
    _run_and_check("wrmf", optname, D, roles)


@pytest.mark.parametrize("optname,D,roles", [(o, D, r) for o in OPTS for D in (50, 64) for r in STRICT_NB])
def test_bias_free_bpr_subset(optname, D, roles):
    _run_and_check("bpr", optname, D, roles, has_bias=False)


@pytest.mark.parametrize("optname", ["adagrad", "adam", "momentum"])
@pytest.mark.parametrize("model", ["bpr", "wrmf"])
def test_frozen_slots_keep_their_bits(model, optname):
    """a full step first, so that every table has slots; then a users-only call: the item and bias tables AND their slots
    are bit-for-bit what they were"""
    rt = _rt()
    D = 64
    U, V, b, uid, pid, nid, lab = _case(5, D, pointwise=model == "wrmf")
    tU = rt.Table(NU, D).write(U); tV = rt.Table(NI, D).write(V); tb = rt.Table(NI, 1).write(b)
    opt, _ = _opts(optname, rt)
    ids = _ids_of(model, uid, pid, nid, lab)
    _device_step(rt, model, opt, tU, tV, tb, tuple(x[:1] for x in ids), 1, None)
    nslot = 2 if optname == "adam" else 1
    before = [tV.read(), tb.read()] + [opt.slot(t, k) for t in (tV, tb) for k in range(nslot)]
    u_before = tU.read()
    _device_step(rt, model, opt, tU, tV, tb, ids, K, ("user",))
    after = [tV.read(), tb.read()] + [opt.slot(t, k) for t in (tV, tb) for k in range(nslot)]
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    assert not np.array_equal(u_before, tU.read())


def _twice_case(seed, D, nu=4000, ni=8000, Bt=2048):
    """every user referenced exactly twice per step, 64 items twice, the others once.  The full step sums the gradients of a row
    referenced three times or more in an order its plan chooses per call, so two runs of the SAME full call differ in the
    last bits on such rows; bit equality of two routes can only be asked where every row has at most two references (the
    inputs tests/test_gpu_momentum.py compares one K-step call with K one-step calls on)"""
    rng = np.random.default_rng(seed)
    U = rng.uniform(-.05, .05, (nu, D)).astype(np.float32); V = rng.uniform(-.05, .05, (ni, D)).astype(np.float32)
    b = rng.uniform(-.05, .05, (ni, 1)).astype(np.float32)
    uid = np.stack([rng.permutation(np.concatenate([u, u])) for u in (rng.permutation(nu)[:Bt // 2] for _ in range(K))]).astype(np.int32)
    items = [rng.permutation(ni)[:2 * Bt - 64] for _ in range(K)]
    items = np.stack([rng.permutation(np.concatenate([it, it[:64]])) for it in items]).astype(np.int32)
    lab = (rng.random((K, Bt)) < 0.3).astype(np.float32)
    return U, V, b, uid, np.ascontiguousarray(items[:, :Bt]), np.ascontiguousarray(items[:, Bt:]), lab


@pytest.mark.parametrize("model", ["bpr", "ucml", "wrmf", "bpr_nb"])
def test_full_mask_is_the_full_step(model):
    """the mask that names every table takes the full step's route: the same bits as the call without `train`"""
    rt = _rt()
    D, Bt = 64, 2048
    nb = model == "bpr_nb"
    m = "bpr" if nb else model
    U, V, b, uid, pid, nid, lab = _twice_case(9, D, Bt=Bt)
    ids = (uid, pid, lab) if m == "wrmf" else (uid, pid, nid)
    res = []
    for train in (None, ("user", "item") if nb else ROLES):
        tU = rt.Table(*U.shape).write(U); tV = rt.Table(*V.shape).write(V); tb = None if nb else rt.Table(*b.shape).write(b)
        opt = rt.Optimizer.adagrad(0.05)
        if m == "wrmf":
            loss, l2 = rt.pointwise_step("wrmf", opt, tU, tV, tb, None, *ids, K=K, B=Bt, a=2.0, b_w=0.5, train=train)
        else:
            loss, l2 = rt.pairwise_step(m, opt, tU, tV, tb, *ids, K=K, B=Bt, margin=0.5, train=train)
        res.append([tU.read(), tV.read(), loss, l2, opt.slot(tU), opt.slot(tV)] + ([] if nb else [tb.read(), opt.slot(tb)]))
    for x, y in zip(*res):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("model,optname,roles", [("bpr", "sgd", ("user",)), ("ucml", "adam", ("item", "bias")), ("wrmf", "momentum", ("user", "bias")),
                                                 ("bpr", "adagrad", ("item",))])
def test_one_k3_call_equals_three_one_step_calls(model, optname, roles):
    _run_and_check(model, optname, 64, roles, split=True, seed=3)


def test_adam_users_only_then_full_steps():
    """three steps users only, then three full steps, against the same sequence in the oracle: a frozen table that took
    decay, or a lazily applied table that was not finished before it was frozen, shows here"""
    from oracle import numpy_oracle as orc
    rt = _rt()
    D = 64
    U, V, b, uid, pid, nid, _ = _case(21, D)
    rng = np.random.default_rng(22)
    uid2, pid2, nid2 = (rng.integers(0, hi, (K, B)).astype(np.int32) for hi in (NU, NI, NI))
    tU = rt.Table(NU, D).write(U); tV = rt.Table(NI, D).write(V); tb = rt.Table(NI, 1).write(b)
    opt = rt.Optimizer.adam(LR["adam"]); oo = orc.AdamTFSparse(LR["adam"])
    # a full step first: the three tables are lazily applied under `opt` when the users-only phase begins
    rt.pairwise_step("bpr", opt, tU, tV, tb, uid2[0], pid2[0], nid2[0], K=1, B=B)
    orc.bpr_step(U, V, b, uid2[0], pid2[0], nid2[0], oo)
    l1, _ = rt.pairwise_step("bpr", opt, tU, tV, tb, uid, pid, nid, K=K, B=B, train=("user",))
    V1, b1 = tV.read(), tb.read()
    for s in range(K):
        lw, _ = _expect_step("bpr", U, V, b, (uid[s], pid[s], nid[s]), oo, ("user",))
        assert abs(l1[s] - lw) <= TOL * abs(lw)
    assert rel_err(V1, V) <= TOL_ADAM and rel_err(b1, b) <= TOL_ADAM and rel_err(tU.read(), U) <= TOL_ADAM
    assert opt.step == 1 + K
    l2_, _ = rt.pairwise_step("bpr", opt, tU, tV, tb, uid2, pid2, nid2, K=K, B=B)
    for s in range(K):
        lw, _ = orc.bpr_step(U, V, b, uid2[s], pid2[s], nid2[s], oo)
        assert abs(l2_[s] - lw) <= TOL * abs(lw)
    assert opt.step == 1 + 2 * K
    for nm, t, want in (("U", tU, U), ("V", tV, V), ("b", tb, b)):
        e = rel_err(t.read(), want)
        print("two-phase Adam", nm, e)
        assert e <= TOL_ADAM, (nm, e)
        em, ev = rel_err(opt.slot(t, 0), oo.m[nm]), rel_err(opt.slot(t, 1), oo.v[nm])
        print("two-phase Adam slots", nm, em, ev)
        assert em <= TOL_ADAM and ev <= TOL_ADAM, (nm, em, ev)


@pytest.mark.parametrize("model", ["bpr", "ucml", "wrmf"])
def test_device_ids_give_the_same_result(model):
    pytest.importorskip("torch")
    # (no full step first: it sums the gradients of a row referenced three times or more in an order its plan chooses per call)
    a, _, _ = _run_and_check(model, "adagrad", 64, ("user", "bias"), seed=13, warm_up=False)
    c, _, _ = _run_and_check(model, "adagrad", 64, ("user", "bias"), seed=13, device_ids=True, warm_up=False)
    for r in ROLES:
        assert np.array_equal(a[r].read(), c[r].read())


def test_c2_sized_users_only_against_the_c_oracle():
    """BPR D = 64, 1M x 1M, B = 65536, SGD, users only, K = 4.  The C oracle only knows the full step; its tables are
    caller-owned arrays, so after each of its steps the rows of V and b the step referenced are put back to their start values:
    under snapshot semantics the user table it leaves is the users-only result."""
    from oracle import c_oracle
    rt = _rt()
    N, Bc, Kc, D = 1_000_000, 65536, 4, 64
    rng = np.random.default_rng(1)
    U = rng.uniform(-.05, .05, (N, D)).astype(np.float32); V = rng.uniform(-.05, .05, (N, D)).astype(np.float32)
    b = rng.uniform(-.05, .05, (N, 1)).astype(np.float32)
    uid, pid, nid = (rng.integers(0, N, (Kc, Bc)).astype(np.int32) for _ in range(3))
    U0, V0, b0 = U.copy(), V.copy(), b.copy()
    tU = rt.Table(N, D).write(U); tV = rt.Table(N, D).write(V); tb = rt.Table(N, 1).write(b)
    loss, l2 = rt.pairwise_step("bpr", rt.Optimizer.sgd(0.05), tU, tV, tb, uid, pid, nid, K=Kc, B=Bc, train=("user",))
    cpu = c_oracle.PairwiseCPU("bpr", "sgd", U, V, b, lr=0.05)
    for s in range(Kc):
        lw, l2w = cpu.step(uid[s], pid[s], nid[s])
        it = np.concatenate([pid[s], nid[s]])
        V[it] = V0[it]; b[it] = b0[it]
        assert abs(loss[s] - lw) <= 1e-5 * abs(lw) and abs(l2[s] - l2w) <= 1e-5 * abs(l2w)
    coef = delta_check(U0, tU.read(), U, steps=Kc, what="C2 users only")
    assert abs(coef - 1.0) <= 1e-4, coef
    assert np.array_equal(tV.read(), V0) and np.array_equal(tb.read(), b0)


# ---- through the TensorFlow-shaped surface ---------------------------------------------------------------------------------
def _shim_model(kind, D):
    from openrec_amd.tf2.compat import optimizers
    if kind == "composed":
        from compose_models import BPR
    else:
        from openrec_amd.tf2.recommenders import BPR
    model = BPR(D, D, NU, NI)
    return model, optimizers.SGD(0.05)


@pytest.mark.parametrize("kind", ["variables", "trainable", "composed"])
def test_shim_trains_the_users_only_then_everything(kind):
    """33 steps with the user variables only (a queue of 32 flushes once on the way): items and biases keep their bits, users
    follow the oracle; then two steps with the full variable list: the change of mask flushed the queue, the sequence is
    the oracle's"""
    from openrec_amd.tf2.compat import tf
    from oracle import numpy_oracle as orc
    D, S = 16, 33
    model, opt = _shim_model(kind, D)
    U, V, b = (f.variables[0].numpy() for f in (model.user_latent_factor, model.item_latent_factor, model.item_bias))
    V0, b0 = V.copy(), b.copy()
    rng = np.random.default_rng(3)
    ids = [tuple(rng.integers(0, hi, B).astype(np.int32) for hi in (NU, NI, NI)) for _ in range(S + 2)]
    oo = orc.SGD(0.05)
    if kind == "trainable":
        model.item_latent_factor.trainable = False
        model.item_bias.trainable = False
        assert len(model.trainable_variables) == 1 and len(model.variables) == 3

    def train_step(u, p, n, variables):             # tf2_examples/bpr_citeulike.py:33-39
        with tf.GradientTape() as tape:
            loss_value = model(u, p, n)
        gradients = tape.gradient(loss_value, variables)
        opt.apply_gradients(zip(gradients, variables))
        return loss_value

    for s in range(S):
        variables = model.trainable_variables if kind == "trainable" else model.user_latent_factor.variables
        train_step(*ids[s], variables)
        _expect_step("bpr", U, V, b, ids[s], oo, ("user",))
    if kind == "trainable":
        model.item_latent_factor.trainable = True
        model.item_bias.trainable = True
    losses = []
    for s in range(S, S + 2):
        losses.append(train_step(*ids[s], model.trainable_variables))
    got_U, got_V, got_b = (f.variables[0].numpy() for f in (model.user_latent_factor, model.item_latent_factor, model.item_bias))
    for s in range(S, S + 2):
        lw, _ = orc.bpr_step(U, V, b, *ids[s], oo)
        assert abs(float(losses[s - S][0]) - lw) <= TOL * abs(lw)
    assert rel_err(got_U, U) < TOL and rel_err(got_V, V) < TOL and rel_err(got_b, b) < TOL
    # only rows the two full steps referenced may differ from the start: every other item row kept its bits through the 33
    it = np.unique(np.concatenate([np.concatenate(ids[s][1:]) for s in range(S, S + 2)]))
    rest = np.ones(NI, bool); rest[it] = False
    assert rest.any() and np.array_equal(got_V[rest], V0[rest]) and np.array_equal(got_b[rest], b0[rest])


def test_shim_frozen_tables_keep_their_bits_after_33_steps():
    from openrec_amd.tf2.compat import tf
    from oracle import numpy_oracle as orc
    D = 16
    model, opt = _shim_model("variables", D)
    U, V, b = (f.variables[0].numpy() for f in (model.user_latent_factor, model.item_latent_factor, model.item_bias))
    V0, b0 = V.copy(), b.copy()
    rng = np.random.default_rng(5)
    oo = orc.SGD(0.05)
    vars_ = model.user_latent_factor.variables
    for s in range(33):
        u, p, n = (rng.integers(0, hi, B).astype(np.int32) for hi in (NU, NI, NI))
        with tf.GradientTape() as tape:
            loss = model(u, p, n)
        opt.apply_gradients(zip(tape.gradient(loss, vars_), vars_))
        _expect_step("bpr", U, V, b, (u, p, n), oo, ("user",))
    assert np.array_equal(model.item_latent_factor.variables[0].numpy(), V0)
    assert np.array_equal(model.item_bias.variables[0].numpy(), b0)
    assert rel_err(model.user_latent_factor.variables[0].numpy(), U) < TOL


def test_ucml_users_only_then_censor_vec():
    """censor_vec is an assignment, not a gradient: as in Keras it rescales item rows whose table is frozen; the censor of a
    subset step is never folded into the step (it runs as its own calls).  `user_latent_factor.censor` alone leaves the items."""
    from openrec_amd.tf2.compat import tf, optimizers
    from openrec_amd.tf2.recommenders import UCML
    from oracle import numpy_oracle as orc
    D = 16
    model, opt = UCML(D, D, NU, NI), optimizers.SGD(0.05)
    for f in (model.user_latent_factor, model.item_latent_factor):
        f.variables[0].assign(f.variables[0].numpy() * 8.0)        # norms above min_norm = 0.1: the censor rescales the rows
    U, V, b = (f.variables[0].numpy() for f in (model.user_latent_factor, model.item_latent_factor, model.item_bias))
    rng = np.random.default_rng(8)
    oo = orc.SGD(0.05)
    vars_ = model.user_latent_factor.variables
    for s in range(2):
        u, p, n = (rng.integers(0, hi, B).astype(np.int32) for hi in (NU, NI, NI))
        with tf.GradientTape() as tape:
            loss = model(u, p, n)
        opt.apply_gradients(zip(tape.gradient(loss, vars_), vars_))
        _expect_step("ucml", U, V, b, (u, p, n), oo, ("user",))
        if s == 0:
            out = model.censor_vec(u, p, n)
            assert len(out) == 3
            orc.censor(U, u); orc.censor(V, p); orc.censor(V, n)
        else:
            V_before = model.item_latent_factor.variables[0].numpy()
            model.user_latent_factor.censor(u)
            orc.censor(U, u)
            assert np.array_equal(model.item_latent_factor.variables[0].numpy(), V_before)
    assert rel_err(model.user_latent_factor.variables[0].numpy(), U) < TOL
    assert rel_err(model.item_latent_factor.variables[0].numpy(), V) < TOL
    assert np.array_equal(model.item_bias.variables[0].numpy(), b)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_name_their_cause():
    from openrec_amd import _ffi
    rt = _rt()
    D = 16
    U, V, b, uid, pid, nid, lab = _case(2, D)
    tU = rt.Table(NU, D).write(U); tV = rt.Table(NI, D).write(V); tb = rt.Table(NI, 1).write(b)
    tw = rt.Table(D, 1).fill(1.0)
    opt = rt.Optimizer.sgd(0.05)
    lib, ctx = tU.ctx._lib, tU.ctx._h
    u, p, n = (np.ascontiguousarray(x[0]) for x in (uid, pid, nid))
    y = np.ascontiguousarray(lab[0])

    def pair(mask, bias=tb, flags=0, model=_ffi.ORX_BPR):
        return lib.orx_pairwise_step_subset(ctx, model, opt._h, tU._h, tV._h, bias._h if bias is not None else None, u.ctypes.data, p.ctypes.data,
                                            n.ctypes.data, 1, B, B, 0.5, flags, mask, None, None)

    def point(mask, model, flags=0):
        return lib.orx_pointwise_step_subset(ctx, model, opt._h, tU._h, tV._h, tb._h, tw._h if model == _ffi.ORX_GMF else None, u.ctypes.data,
                                             p.ctypes.data, y.ctypes.data, 1, B, B, 1.0, 1.0, flags, mask, None, None)

    def refused(rc, *words):
        assert rc == _ffi.ORX_ERR_ARG, rc
        msg = lib.orx_last_error().decode()
        assert all(w in msg for w in words), msg

    before = tU.read()
    refused(pair(0), "empty train mask")
    refused(pair(8), "bits outside")
    refused(pair(_ffi.ORX_TRAIN_USER | _ffi.ORX_TRAIN_BIAS, bias=None), "ORX_TRAIN_BIAS", "bias")
    refused(pair(_ffi.ORX_TRAIN_USER, flags=_ffi.ORX_HOGWILD), "ORX_HOGWILD")
    refused(pair(_ffi.ORX_TRAIN_USER, flags=_ffi.ORX_CENSOR, model=_ffi.ORX_UCML), "ORX_CENSOR")
    refused(point(0, _ffi.ORX_WRMF), "empty train mask")
    refused(point(_ffi.ORX_TRAIN_ITEM, _ffi.ORX_GMF), "ORX_GMF", "fourth role")
    refused(point(_ffi.ORX_TRAIN_ITEM, _ffi.ORX_WRMF, flags=_ffi.ORX_HOGWILD), "ORX_HOGWILD")
    assert np.array_equal(tU.read(), before)
    with pytest.raises(IndexError):
        bad = u.copy(); bad[5] = NU
        rt.pairwise_step("bpr", opt, tU, tV, tb, bad, p, n, train=("user",))
    with pytest.raises(IndexError):
        bad = p.copy(); bad[7] = -1          # an id of a FROZEN table: checked by the gradient launch all the same
        rt.pairwise_step("bpr", opt, tU, tV, tb, u, bad, n, train=("user",))


def test_shim_refusals():
    from openrec_amd.tf2.compat import tf, optimizers
    from openrec_amd.tf2.recommenders import BPR, GMF
    D = 16
    rng = np.random.default_rng(4)
    u, p, n = (rng.integers(0, hi, B).astype(np.int32) for hi in (NU, NI, NI))
    model, other = BPR(D, D, NU, NI), BPR(D, D, NU, NI)
    opt = optimizers.SGD(0.05)
    with tf.GradientTape() as tape:
        loss = model(u, p, n)
    vars_ = other.user_latent_factor.variables
    with pytest.raises(ValueError, match="user_latent_factor"):
        opt.apply_gradients(zip(tape.gradient(loss, vars_), vars_))
    gmf = GMF(D, D, NU, NI)
    y = (rng.random(B) < 0.3).astype(np.float32)
    with tf.GradientTape() as tape:
        loss = gmf(u, p, y)
    vars_ = gmf.user_latent_factor.variables
    with pytest.raises(NotImplementedError, match="GMF"):
        opt.apply_gradients(zip(tape.gradient(loss, vars_), vars_))


@pytest.mark.parametrize("kind", ["packaged", "composed"])
def test_dlrm_refuses_a_strict_subset_and_a_foreign_variable(kind):
    """the packaged DLRM hands out its own variables, a DLRM composed by hand from the modules hands out the modules': both are
    matched by table, a strict subset (embeddings only, MLPs only) names the model and what is missing, nothing is trained"""
    from openrec_amd.tf2 import compat
    from openrec_amd.tf2.compat import tf, optimizers
    from openrec_amd.tf2.recommenders import BPR
    cfg = dict(m_spa=16, ln_emb=[50, 7, 30], ln_bot=[32, 16], ln_top=[64, 32, 1])
    if kind == "composed":
        compat.install()
        import compose_models
        model = compose_models.DLRM(loss_func="mse", loss_threshold=0.0, **cfg)
    else:
        from openrec_amd.tf2.recommenders import DLRM
        model = DLRM(**cfg)
    rng = np.random.default_rng(6)
    Bd = 64
    d = np.log1p(rng.integers(0, 100, (Bd, 13))).astype(np.float32)
    s = np.stack([rng.integers(0, n, Bd) for n in cfg["ln_emb"]], 1).astype(np.int32)
    y = (rng.random(Bd) < 0.3).astype(np.float32)
    opt = optimizers.SGD(0.05)
    float(model(d, s, y))                       # (a composition binds its modules to the fused step at its first call)
    every = list(model.trainable_variables)
    before = [v.numpy() for v in every]
    n_emb = len(cfg["ln_emb"]) if kind == "composed" else 1
    for subset, word in ((every[:n_emb], "dense"), (every[n_emb:], "embeddings"), (every[1:], "embeddings") if kind == "composed" else (every[:2], "dense")):
        with tf.GradientTape() as tape:
            loss = model(d, s, y)
        with pytest.raises(NotImplementedError, match="DLRM") as e:
            opt.apply_gradients(zip(tape.gradient(loss, subset), subset))
        assert word in str(e.value), str(e.value)
    other = BPR(16, 16, 50, 60)
    with tf.GradientTape() as tape:
        loss = model(d, s, y)
    vars_ = every + other.user_latent_factor.variables
    with pytest.raises(ValueError, match="user_latent_factor"):
        opt.apply_gradients(zip(tape.gradient(loss, vars_), vars_))
    for v, w in zip(every, before):
        assert np.array_equal(v.numpy(), w)
    with tf.GradientTape() as tape:             # the full list is the step there is
        loss = model(d, s, y)
    opt.apply_gradients(zip(tape.gradient(loss, every), every))
    assert any(not np.array_equal(v.numpy(), w) for v, w in zip(every, before))
