"""SGD with momentum / Nesterov (keras.optimizers.SGD(lr, momentum > 0, nesterov)) on the device: every single-GPU train step
(pairwise BPR / UCML, pointwise GMF / WRMF, orx_apply_rows, DLRM) against the NumPy restatement tests/keras_momentum.py, which
drives the oracle's train steps unchanged.  Tables are held to conftest.delta_check (parity of the UPDATE), losses and the
velocity slot to TOL.  The refusals (hogwild, the sharded entry points) name momentum; the C ABI reports them as ORX_ERR_ARG,
which the Python layer raises as ValueError."""
import os
import tempfile

import numpy as np
import pytest

from conftest import TOL, delta_check, rel_err
from keras_momentum import Momentum

pytestmark = pytest.mark.gpu

LR, MOM = 0.05, 0.9


def _rt():
    from openrec_amd import runtime as rt
    return rt


def _pair_case(seed, NU, NI, B, D, K):
    """batches heavy in duplicates: rows referenced exactly twice and >= 3 times, p == n, boundary ids"""
    rng = np.random.default_rng(seed)
    U = rng.uniform(-.05, .05, (NU, D)).astype(np.float32)
    V = rng.uniform(-.05, .05, (NI, D)).astype(np.float32)
    b = rng.uniform(-.05, .05, (NI, 1)).astype(np.float32)
    uid = rng.integers(0, NU, (K, B)).astype(np.int32)
    pid = rng.integers(0, NI, (K, B)).astype(np.int32)
    nid = rng.integers(0, NI, (K, B)).astype(np.int32)
    uid[:, :2] = 7                                   # user 7 exactly twice (NU is large: no other reference is likely)
    uid[:, 2:14] = 3                                 # user 3 twelve times
    pid[:, 20:22] = 5; nid[:, 30] = 5                # item 5 three times, as positive and negative
    nid[:, 40:60] = pid[:, 40:60]                    # p == n
    uid[:, -1], pid[:, -1], nid[:, -1] = NU - 1, NI - 1, 0
    return U, V, b, uid, pid, nid


def _check_pair(rt, model, censor, D, nesterov, K, uid, pid, nid, U, V, b, tol_loss=TOL, lr=LR):
    from oracle import numpy_oracle as orc
    B = uid.shape[1]
    U0, V0, b0 = U.copy(), V.copy(), b.copy()
    tU = rt.Table(*U.shape).write(U); tV = rt.Table(*V.shape).write(V); tb = rt.Table(*b.shape).write(b)
    opt = rt.Optimizer.momentum(lr, MOM, nesterov)
    loss, l2 = rt.pairwise_step(model, opt, tU, tV, tb, uid, pid, nid, K=K, B=B, margin=0.5, censor=censor)
    oo = Momentum(lr, MOM, nesterov)
    for s in range(K):
        if model == "bpr":
            lr_, l2r = orc.bpr_step(U, V, b, uid[s], pid[s], nid[s], oo)
        else:
            lr_, l2r = orc.ucml_step(U, V, b, uid[s], pid[s], nid[s], oo, margin=0.5, do_censor=censor)
        assert abs(loss[s] - lr_) <= tol_loss * abs(lr_) and abs(l2[s] - l2r) <= tol_loss * abs(l2r), (s, loss[s], lr_)
    what = f"{model} censor={censor} D={D} nesterov={nesterov} K={K}"
    if censor:
        # censor_vec rescales a row by 1 / ||row||: the table is compared whole (the rescale is no update of the rule's size)
        assert rel_err(tU.read(), U) < TOL and rel_err(tV.read(), V) < TOL and rel_err(tb.read(), b) < TOL, what
    else:
        for nm, w0, got, want in (("U", U0, tU.read(), U), ("V", V0, tV.read(), V), ("b", b0, tb.read(), b)):
            delta_check(w0, got, want, steps=K, what=f"{what} {nm}")
    for nm, t in (("U", tU), ("V", tV), ("b", tb)):
        assert rel_err(opt.slot(t, 0), oo.vel[nm]) < TOL, (what, nm)
    return tU, tV, tb, opt


PAIR_CASES = [(m, c, D, n, K) for (m, c) in (("bpr", False), ("ucml", False), ("ucml", True)) for D in (16, 64, 128, 50)
              for n in (False, True) for K in (1, 20)]


@pytest.mark.parametrize("model,censor,D,nesterov,K", PAIR_CASES)
def test_pairwise_momentum_matches_the_restatement(model, censor, D, nesterov, K):
    rt = _rt()
    U, V, b, uid, pid, nid = _pair_case(11 + D + K, 20000, 3000, 1024, D, K)
    _check_pair(rt, model, censor, D, nesterov, K, uid, pid, nid, U, V, b)


@pytest.mark.parametrize("model", ["bpr", "ucml"])
@pytest.mark.parametrize("nesterov", [False, True])
def test_pairwise_momentum_all_same_user(model, nesterov):
    rt = _rt()
    U, V, b, uid, pid, nid = _pair_case(4, 10, 3000, 1024, 64, 3)
    uid[:] = 4
    # the user row sums 1024 gradients: lr * 1024 < 1, or the row's own l2 term makes the three steps diverge
    _check_pair(rt, model, False, 64, nesterov, 3, uid, pid, nid, U, V, b, lr=5e-4)


@pytest.mark.parametrize("fallback", ["1", "2", "4", "8"])
@pytest.mark.parametrize("model,censor,D", [("bpr", False, 64), ("ucml", True, 128), ("ucml", False, 16)])
def test_pairwise_momentum_fallback_routes(fallback, model, censor, D, monkeypatch):
    """ORX_FORCE_FALLBACK: 1 = no role bits (atomics, separate dup_apply launches), 2 = no in-launch apply,
    4 = separate censor passes, 8 = atomics instead of staging slots"""
    monkeypatch.setenv("ORX_FORCE_FALLBACK", fallback)
    rt = _rt()
    for nesterov in (False, True):
        U, V, b, uid, pid, nid = _pair_case(21 + D, 20000, 3000, 1024, D, 6)
        _check_pair(rt, model, censor, D, nesterov, 6, uid, pid, nid, U, V, b)


def _twice_case(seed, K, B, D, NU, NI):
    """every user referenced exactly twice per step, 64 items twice, the others once: no row of >= 3 references, whose
    gradients are summed in an order that depends on the plan of the call (for every optimizer)"""
    rng = np.random.default_rng(seed)
    U = rng.uniform(-.05, .05, (NU, D)).astype(np.float32); V = rng.uniform(-.05, .05, (NI, D)).astype(np.float32)
    b = rng.uniform(-.05, .05, (NI, 1)).astype(np.float32)
    uid = np.stack([rng.permutation(np.concatenate([u, u])) for u in (rng.permutation(NU)[:B // 2] for _ in range(K))]).astype(np.int32)
    items = [rng.permutation(NI)[:2 * B - 64] for _ in range(K)]
    items = np.stack([rng.permutation(np.concatenate([it, it[:64]])) for it in items]).astype(np.int32)
    return U, V, b, uid, np.ascontiguousarray(items[:, :B]), np.ascontiguousarray(items[:, B:])


@pytest.mark.parametrize("optname", ["adagrad", "momentum"])
def test_one_k20_call_equals_twenty_single_step_calls(optname):
    """one K = 20 call (duplicated rows applied inside the next step's launch, tail launch) and 20 one-step calls (dup_apply
    launches): bit-identical tables and slots, for momentum as for Adagrad (rows referenced at most twice: _twice_case)"""
    rt = _rt()
    K, B = 20, 2048
    U, V, b, uid, pid, nid = _twice_case(5, K, B, 64, 4000, 8000)
    res = []
    for split in (False, True):
        tU = rt.Table(*U.shape).write(U); tV = rt.Table(*V.shape).write(V); tb = rt.Table(*b.shape).write(b)
        opt = rt.Optimizer.adagrad(LR) if optname == "adagrad" else rt.Optimizer.momentum(LR, MOM, True)
        if split:
            for s in range(K):
                rt.pairwise_step("bpr", opt, tU, tV, tb, uid[s], pid[s], nid[s], K=1, B=B)
        else:
            rt.pairwise_step("bpr", opt, tU, tV, tb, uid, pid, nid, K=K, B=B)
        res.append([tU.read(), tV.read(), tb.read(), opt.slot(tU), opt.slot(tV), opt.slot(tb)])
    for a, c in zip(*res):
        assert np.array_equal(a, c)


@pytest.mark.parametrize("model,D,nowtail,sigmoid", [("gmf", 64, False, False), ("gmf", 64, True, False), ("gmf", 50, False, False),
                                                     ("wrmf", 32, False, False), ("wrmf", 64, False, True), ("wrmf", 50, False, True)])
@pytest.mark.parametrize("nesterov", [False, True])
def test_pointwise_momentum_matches_the_restatement(model, D, nowtail, sigmoid, nesterov, monkeypatch):
    """GMF: the Dense(1) kernel's dense rule in the reducer workgroups of the step's launch, or (ORX_POINT_NO_WTAIL=1) in the
    reduce launch; WRMF with and without the sigmoid"""
    if nowtail:
        monkeypatch.setenv("ORX_POINT_NO_WTAIL", "1")
    rt = _rt()
    from oracle import numpy_oracle as orc
    NU, NI, B, K = 5000, 3000, 2048, 4
    rng = np.random.default_rng(8 + D)
    U = rng.uniform(-.05, .05, (NU, D)).astype(np.float32); V = rng.uniform(-.05, .05, (NI, D)).astype(np.float32)
    b = rng.uniform(-.05, .05, (NI, 1)).astype(np.float32); wk = rng.uniform(-.3, .3, (D, 1)).astype(np.float32)
    uid = rng.integers(0, NU, (K, B)).astype(np.int32); iid = rng.integers(0, NI, (K, B)).astype(np.int32)
    uid[:, :40] = 11; iid[:, 40:43] = 9
    lab = (rng.random((K, B)) < 0.4).astype(np.float32)
    U0, V0, b0, w0 = U.copy(), V.copy(), b.copy(), wk.copy()
    tU = rt.Table(NU, D).write(U); tV = rt.Table(NI, D).write(V); tb = rt.Table(NI, 1).write(b)
    tw = rt.Table(D, 1).write(wk) if model == "gmf" else None
    opt = rt.Optimizer.momentum(LR, MOM, nesterov)
    oo = Momentum(LR, MOM, nesterov)
    kw = dict(a=2.0, b_w=0.5)
    if model == "wrmf":
        kw["sigmoid"] = sigmoid
    loss, l2 = rt.pointwise_step(model, opt, tU, tV, tb, tw, uid, iid, lab, K=K, B=B, **kw)
    for s in range(K):
        if model == "gmf":
            lw, l2w = orc.gmf_step(U, V, b, wk, uid[s], iid[s], lab[s], oo)
        else:
            lw, l2w = orc.wrmf_step(U, V, b, uid[s], iid[s], lab[s], oo, a=2.0, b_w=0.5, sigmoid=sigmoid)
        assert abs(loss[s] - lw) <= TOL * abs(lw) and abs(l2[s] - l2w) <= TOL * abs(l2w), (s, loss[s], lw)
    for nm, x0, got, want in (("U", U0, tU.read(), U), ("V", V0, tV.read(), V), ("b", b0, tb.read(), b)):
        delta_check(x0, got, want, steps=K, what=f"{model} D={D} {nm}")
        assert rel_err(opt.slot({"U": tU, "V": tV, "b": tb}[nm], 0), oo.vel[nm]) < TOL, nm
    if model == "gmf":
        # the Dense(1) gradient is a sum over the whole batch (2048 terms, reduced in a different order than NumPy's)
        assert rel_err(tw.read(), wk) < TOL and rel_err(opt.slot(tw, 0), oo.vel["w"]) < 1e-4


@pytest.mark.parametrize("D,bias,atomics", [(64, False, False), (50, False, False), (64, True, False), (300, False, False), (64, False, True)])
@pytest.mark.parametrize("nesterov", [False, True])
def test_apply_rows_momentum(D, bias, atomics, nesterov, monkeypatch):
    """orx_apply_rows: the sorted deterministic path (no bias, dim <= 256), the flagged path with dup_apply (a bias column,
    wider rows, ORX_ROWS_ATOMICS=1)"""
    if atomics:
        monkeypatch.setenv("ORX_ROWS_ATOMICS", "1")
    rt = _rt()
    import torch
    from openrec_amd._ffi import check
    ctx = rt.default_context(); lib = ctx._lib
    rng = np.random.default_rng(D)
    R, n = 500, 3000
    W = rng.uniform(-.05, .05, (R, D)).astype(np.float32); bb = rng.uniform(-.05, .05, (R, 1)).astype(np.float32)
    t = rt.Table(R, D).write(W); tb = rt.Table(R, 1).write(bb) if bias else None
    opt = rt.Optimizer.momentum(LR, MOM, nesterov)
    oo = Momentum(LR, MOM, nesterov)
    W0, b0 = W.copy(), bb.copy()
    for s in range(3):
        ids = rng.integers(0, R, n).astype(np.int32)
        g = rng.normal(size=(n, D + (1 if bias else 0))).astype(np.float32) * 0.01
        di = torch.from_numpy(ids).to("cuda:0"); dg = torch.from_numpy(g).to("cuda:0")
        torch.cuda.synchronize()
        check(lib.orx_apply_rows(ctx._h, opt._h, t._h, tb._h if bias else None, di.data_ptr(), n, dg.data_ptr(), dg.shape[1]))
        oo.apply(W, ids, g[:, :D], key="W")
        if bias:
            oo.apply(bb, ids, g[:, D:], key="b")
    delta_check(W0, t.read(), W, steps=3, what="apply_rows W")
    assert rel_err(opt.slot(t, 0), oo.vel["W"]) < TOL
    if bias:
        delta_check(b0, tb.read(), bb, steps=3, what="apply_rows b")
        assert rel_err(opt.slot(tb, 0), oo.vel["b"]) < TOL


def test_checkpoint_resume_is_bit_identical():
    rt = _rt()
    K, B = 6, 1024
    U, V, b, uid, pid, nid = _twice_case(9, K, B, 64, 3000, 3000)

    def fresh():
        return (rt.Table(*U.shape).write(U), rt.Table(*V.shape).write(V), rt.Table(*b.shape).write(b),
                rt.Optimizer.momentum(LR, MOM, True))
    tU, tV, tb, opt = fresh()
    rt.pairwise_step("bpr", opt, tU, tV, tb, uid, pid, nid, K=K, B=B)
    straight = [tU.read(), tV.read(), tb.read(), opt.slot(tU), opt.slot(tV), opt.slot(tb)]
    for form in ("dir", "ckpt.npz"):
        tU, tV, tb, opt = fresh()
        rt.pairwise_step("bpr", opt, tU, tV, tb, uid[:3], pid[:3], nid[:3], K=3, B=B)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, form)
            tabs = dict(U=tU, V=tV, b=tb)
            rt.save_checkpoint(path, tabs, opt)
            tU, tV, tb, opt = fresh()
            tU.write(np.zeros_like(U))
            rt.load_checkpoint(path, dict(U=tU, V=tV, b=tb), opt)
            with pytest.raises(ValueError, match="momentum"):
                rt.load_checkpoint(path, dict(U=tU, V=tV, b=tb), rt.Optimizer.momentum(LR, 0.5, True))
            with pytest.raises(ValueError, match="nesterov"):
                rt.load_checkpoint(path, dict(U=tU, V=tV, b=tb), rt.Optimizer.momentum(LR, MOM, False))
        rt.pairwise_step("bpr", opt, tU, tV, tb, uid[3:], pid[3:], nid[3:], K=3, B=B)
        resumed = [tU.read(), tV.read(), tb.read(), opt.slot(tU), opt.slot(tV), opt.slot(tb)]
        for a, c in zip(straight, resumed):
            assert np.array_equal(a, c), form


def test_learning_rate_change_keeps_the_velocity():
    rt = _rt()
    from oracle import numpy_oracle as orc
    B, D = 1024, 32
    U, V, b, uid, pid, nid = _pair_case(13, 3000, 3000, B, D, 4)
    U0, V0, b0 = U.copy(), V.copy(), b.copy()
    tU = rt.Table(*U.shape).write(U); tV = rt.Table(*V.shape).write(V); tb = rt.Table(*b.shape).write(b)
    opt = rt.Optimizer.momentum(LR, MOM)
    oo = Momentum(LR, MOM)
    for s in range(4):
        if s == 2:
            opt.set_lr(0.01); oo.lr = 0.01
        rt.pairwise_step("bpr", opt, tU, tV, tb, uid[s], pid[s], nid[s], K=1, B=B)
        orc.bpr_step(U, V, b, uid[s], pid[s], nid[s], oo)
    for nm, w0, got, want in (("U", U0, tU.read(), U), ("V", V0, tV.read(), V), ("b", b0, tb.read(), b)):
        delta_check(w0, got, want, steps=4, what=nm)
    assert rel_err(opt.slot(tV), oo.vel["V"]) < TOL


@pytest.mark.parametrize("nesterov", [False, True])
def test_compat_bpr_train_step_with_keras_sgd_momentum(nesterov):
    """the package's BPR recommender trained by a tape-style train_step with tf.keras.optimizers.SGD(0.05, momentum=0.9); the
    learning rate changes between steps 2 and 3"""
    from openrec_amd.tf2 import compat
    compat.install()
    import tensorflow as tf
    from openrec.tf2.recommenders import BPR
    from oracle import numpy_oracle as orc
    NU, NI, D, B = 700, 900, 32, 1024
    model = BPR(dim_user_embed=D, dim_item_embed=D, total_users=NU, total_items=NI)
    opt = tf.keras.optimizers.SGD(0.05, momentum=0.9, nesterov=nesterov)
    assert opt.momentum == pytest.approx(0.9) and opt.nesterov is nesterov

    @tf.function
    def train_step(*batch):
        with tf.GradientTape() as tape:
            loss_value = model(*batch)
        gradients = tape.gradient(loss_value, model.trainable_variables)
        opt.apply_gradients(zip(gradients, model.trainable_variables))
        return loss_value

    U, V, b = (np.array(v.numpy()) for v in model.trainable_variables)
    U0, V0, b0 = U.copy(), V.copy(), b.copy()
    oo = Momentum(0.05, 0.9, nesterov)
    rng = np.random.default_rng(5)
    out, want = [], []
    for it in range(5):
        if it == 2:
            opt.learning_rate = 0.02
            oo.lr = 0.02
        u, p, n = (rng.integers(0, hi, B).astype(np.int32) for hi in (NU, NI, NI))
        out.append(train_step(u, p, n))
        want.append(orc.bpr_step(U, V, b, u, p, n, oo))
    assert opt.native().kind == "momentum"
    for (loss, l2), (lr_, l2r) in zip(out, want):
        assert abs(float(loss) - lr_) <= TOL * abs(lr_) and abs(float(l2) - l2r) <= TOL * abs(l2r)
    got = [np.asarray(v.numpy()) for v in model.trainable_variables]
    for nm, w0, g, w in zip("UVb", (U0, V0, b0), got, (U, V, b)):
        delta_check(w0, g.reshape(w.shape), w, steps=5, what=f"compat BPR {nm}")


def _dlrm_case(nesterov, runs=2, seed=3):
    """exact-mode DLRM, three steps from the same start: the fp64 oracle driven by the restatement, and `runs` device runs"""
    import copy
    from dlrm_util import draw_batch, load_model, round_to_fp32, snapshot
    from oracle.dlrm_oracle import DLRMOracle
    rt = _rt()
    rng = np.random.default_rng(seed)
    ln_emb = [int(x) for x in rng.integers(3, 3000, 8)]
    ln_emb[0], ln_emb[-1] = 3, 40                    # tables of 3 and 40 rows: hundreds of gradient rows per table row
    cfg = dict(m_spa=64, ln_emb=ln_emb, ln_bot=[48, 64], ln_top=[96, 32, 1], dense_dim=13)
    kw = dict(reference_compat=False, loss_func="bce")
    o = round_to_fp32(DLRMOracle(dtype=np.float64, seed=seed + 1, **cfg, **kw))
    o0 = copy.deepcopy(o)
    oo = Momentum(0.05, MOM, nesterov)
    batches, ref = [], []
    for s in range(3):
        bt = draw_batch(o, rng, 777, cfg["ln_emb"], dense_dim=cfg["dense_dim"])
        batches.append(bt)
        ref.append(o.step(*bt, oo))

    def run():
        m = rt.DLRMModel(**cfg, **kw)
        load_model(m, o0)
        opt = rt.Optimizer.momentum(0.05, MOM, nesterov)
        losses = [m.step(opt, *bt)[0] for bt in batches]
        return np.array(losses), snapshot(m, o0, opt)
    return o0, o, ref, [run() for _ in range(runs)]


@pytest.mark.parametrize("route", ["sorted", "atomics"])
@pytest.mark.parametrize("nesterov", [False, True])
def test_dlrm_momentum_exact_mode(nesterov, route, monkeypatch):
    """exact fp32 mode against the fp64 DLRMOracle driven by the restatement.  "sorted": the deterministic sorted sparse apply,
    run twice, bit for bit.  "atomics" (ORX_ROWS_ATOMICS=1, the route of rows wider than 256): duplicate flags + gsum + dup_apply
    (orx_summed_rows_apply); its duplicated rows are summed by fp32 atomics in arrival order, so there is no bit-identity to ask"""
    from dlrm_util import assert_same_bits, assert_updates, params_of
    if route == "atomics":
        monkeypatch.setenv("ORX_ROWS_ATOMICS", "1")
    o0, o, ref, runs = _dlrm_case(nesterov, runs=2 if route == "sorted" else 1)
    l1, s1 = runs[0]
    if route == "sorted":
        assert_same_bits(s1, runs[1][1])
        assert np.array_equal(l1, runs[1][0])
    assert np.abs(l1 - np.array(ref)).max() <= TOL * np.abs(ref).max()
    start = {k: v.astype(np.float32) for k, v in params_of(o0).items()}
    assert_updates(start, s1, params_of(o), TOL, what=f"dlrm momentum nesterov={nesterov} {route}", steps=3)


@pytest.mark.parametrize("variant", [{}, {"ORX_DLRM_FINISH_LAUNCH": "1"}, {"ORX_DLRM_NO_FUSED_DENSE": "1"}],
                         ids=["carried-finish", "finish-launch", "multi-dense"])
def test_dlrm_momentum_fp16_mlp_mode(variant):
    """fp16-MLP mode (the C5 route) with plain and Nesterov momentum against the fp16-operand oracle, with test_gpu_dlrm.py's fp16
    bounds, free-running twice bit for bit (tests/dlrm_momentum_worker.py).  Default: the fused dense optimizer launch carrying the
    sorted apply's finish pass (dense_apply_fused_kernel<true>, CSR_MOMENTUM); ORX_DLRM_FINISH_LAUNCH=1: the finish pass as a launch
    of its own; ORX_DLRM_NO_FUSED_DENSE=1: the multi-tensor dense apply.  One process per variant (the switches are read once)."""
    import subprocess
    import sys as _sys
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dlrm_momentum_worker.py")
    env = dict(os.environ); env.update(variant)
    r = subprocess.run([_sys.executable, worker], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), f"{variant}: {r.stdout[-1500:]} {r.stderr[-3000:]}"


@pytest.mark.parametrize("nesterov", [False, True])
def test_compat_dlrm_train_step_with_keras_sgd_momentum(nesterov):
    """the package's DLRM recommender trained by a tape-style train_step with tf.keras.optimizers.SGD(0.05, momentum=0.9) for five
    steps (queued into one device call); the learning rate changes between steps 2 and 3"""
    import copy
    from openrec_amd.tf2 import compat
    compat.install()
    import tensorflow as tf
    from openrec.tf2.recommenders import DLRM
    from oracle.dlrm_oracle import DLRMOracle
    from dlrm_util import assert_updates, draw_batch, load_model, params_of, round_to_fp32, snapshot
    cfg = dict(m_spa=16, ln_emb=[50, 7, 300, 3], ln_bot=[32, 16], ln_top=[64, 32, 1])
    model = DLRM(loss_func="bce", reference_compat=False, **cfg)
    o = round_to_fp32(DLRMOracle(dtype=np.float64, seed=2, reference_compat=False, loss_func="bce", dense_dim=13, **cfg))
    load_model(model._model, o)                      # the model starts from the oracle's parameters
    o0 = copy.deepcopy(o)
    opt = tf.keras.optimizers.SGD(0.05, momentum=0.9, nesterov=nesterov)

    @tf.function
    def train_step(*batch):
        with tf.GradientTape() as tape:
            loss_value = model(*batch)
        gradients = tape.gradient(loss_value, model.trainable_variables)
        opt.apply_gradients(zip(gradients, model.trainable_variables))
        return loss_value

    oo = Momentum(0.05, 0.9, nesterov)
    rng = np.random.default_rng(11)
    got, want = [], []
    for it in range(5):
        if it == 2:
            opt.learning_rate = 0.02
            oo.lr = 0.02
        de, sp, la = draw_batch(o, rng, 256, cfg["ln_emb"])
        got.append(train_step(de, sp, la))
        want.append(float(o.step(de, sp, la, oo)))
    model.flush()
    assert opt.native().kind == "momentum"
    assert np.allclose([float(g) for g in got], want, rtol=TOL)
    start = {k: v.astype(np.float32) for k, v in params_of(o0).items()}
    assert_updates(start, snapshot(model._model, o), params_of(o), TOL, what=f"compat DLRM nesterov={nesterov}", steps=5)


def test_hogwild_refuses_momentum():
    rt = _rt()
    U, V, b, uid, pid, nid = _pair_case(1, 1000, 1000, 256, 64, 1)
    tU = rt.Table(*U.shape).write(U); tV = rt.Table(*V.shape).write(V); tb = rt.Table(*b.shape).write(b)
    opt = rt.Optimizer.momentum(LR, MOM)
    with pytest.raises(ValueError, match="momentum"):
        rt.pairwise_step("bpr", opt, tU, tV, tb, uid, pid, nid, hogwild=True)
    lab = np.ones(256, np.float32)
    with pytest.raises(ValueError, match="momentum"):
        rt.pointwise_step("wrmf", opt, tU, tV, tb, None, uid[0], pid[0], lab, hogwild=True)
    assert np.array_equal(tU.read(), U)               # nothing was computed


def test_bad_momentum_hyperparameters_are_refused():
    rt = _rt()
    for p0, p1 in ((1.5, 0.0), (-0.1, 0.0), (0.9, 0.5)):
        with pytest.raises(ValueError):
            rt.Optimizer("momentum", 0.01, p0, p1)
    opt = rt.Optimizer.momentum(0.01, 0.9)
    t = rt.Table(10, 4).init_uniform(seed=1)
    assert np.array_equal(opt.slot(t, 0), np.zeros((10, 4), np.float32))     # the velocity starts at zero
    with pytest.raises(ValueError):
        opt.slot(t, 1)


def test_sharded_entry_points_refuse_momentum():
    """the Python engines, and the C entry points themselves: each refuses a momentum optimizer before it looks at anything else"""
    import torch
    from openrec_amd import sharded, sharded_dlrm
    from openrec_amd._ffi import check
    dev = torch.device("cuda", 0)
    with pytest.raises(ValueError, match="momentum"):
        sharded.HipBackend(dev, "momentum", 0.01)
    with pytest.raises(ValueError, match="momentum"):
        sharded_dlrm.HipDLRMBackend(dev, dict(m_spa=16, ln_emb=[10, 20], ln_bot=[16, 16], ln_top=[16, 1], dense_dim=13), "momentum", 0.01)
    rt = _rt()
    lib = rt.default_context()._lib
    opt = rt.Optimizer.momentum(0.01, 0.9)
    calls = {
        "orx_sharded_pairwise_steps": lambda f: f(None, opt._h, 0, *[None] * 6, 1, 1, 1, 1, 1, 0.5, 1.0, 1, 0, None, None),
        "orx_sharded_pairwise_steps_hot": lambda f: f(None, opt._h, 0, *[None] * 5, 0, 1.0, *[None] * 3, 1, 1, 1, 1, 1, 0.5, 1.0, 1, 0,
                                                      None, None),
        "orx_sharded_dlrm_steps": lambda f: f(None, None, opt._h, *[None] * 4, 1, 1, 1.0, None, None),
        "orx_shard_grads_sgd": lambda f: f(None, 0, opt._h, *[None] * 10, 1, 1, 1, 0.5, 0, None, None, None, None),
        "orx_apply_rows_flagged": lambda f: f(None, opt._h, None, None, None, 0, None, 1, None),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="momentum"):
            check(call(getattr(lib, name)))


def test_full_size_bpr_momentum():
    """BPR at configs[1] sizes (1M x 1M, D = 64, B = 65536), three steps of momentum 0.9 in one call"""
    rt = _rt()
    from oracle import numpy_oracle as orc
    NU = NI = 1_000_000
    B, K, D = 65536, 3, 64
    rng = np.random.default_rng(17)
    U = rng.uniform(-.05, .05, (NU, D)).astype(np.float32); V = rng.uniform(-.05, .05, (NI, D)).astype(np.float32)
    b = rng.uniform(-.05, .05, (NI, 1)).astype(np.float32)
    uid = rng.integers(0, NU, (K, B)).astype(np.int32); pid = rng.integers(0, NI, (K, B)).astype(np.int32)
    nid = rng.integers(0, NI, (K, B)).astype(np.int32)
    U0, V0, b0 = U.copy(), V.copy(), b.copy()
    tU = rt.Table(NU, D).write(U); tV = rt.Table(NI, D).write(V); tb = rt.Table(NI, 1).write(b)
    opt = rt.Optimizer.momentum(LR, MOM)
    loss, _ = rt.pairwise_step("bpr", opt, tU, tV, tb, uid, pid, nid, K=K, B=B)
    oo = Momentum(LR, MOM)
    for s in range(K):
        lr_, _ = orc.bpr_step(U, V, b, uid[s], pid[s], nid[s], oo)
        assert abs(loss[s] - lr_) <= TOL * abs(lr_)
    for nm, w0, got, want in (("U", U0, tU.read(), U), ("V", V0, tV.read(), V), ("b", b0, tb.read(), b)):
        coef = delta_check(w0, got, want, steps=K, what=f"full-size {nm}")
        assert abs(coef - 1.0) <= 1e-3, (nm, coef)
