"""BPR without item biases (the reference's PairwiseLogLoss with p_item_bias = n_item_bias = None, score u.p - u.n) on the
device: runtime.pairwise_step / pairwise_loss / score_all_items / rank_metrics with bias=None, and BPR(use_item_bias=False).

Expected values come from a restatement, not from a new oracle: the bias enters only the score and the l2 term covers only the
three row lookups, so for U and V one bias-free step IS one step of the biased model whose bias rows are all zero when the step
starts.  The existing oracles run unchanged with a zero bias table that is set back to zero after every step; only U, V (and
their optimizer slots) are compared."""
import os
import tempfile

import numpy as np
import pytest

from conftest import TOL, TOL_ADAM, delta_check, rel_err
from keras_momentum import Momentum

pytestmark = pytest.mark.gpu

LR = 0.05
OPTS = ("sgd", "adagrad", "momentum", "nesterov", "adam")


def _rt():
    from openrec_amd import runtime as rt
    return rt


def _pair_case(seed, NU, NI, B, D, K):
    """batches heavy in duplicates: rows referenced exactly twice (pairing) and >= 3 times (staging, hot reduce), p == n, boundary ids"""
    rng = np.random.default_rng(seed)
    U = rng.uniform(-.05, .05, (NU, D)).astype(np.float32)
    V = rng.uniform(-.05, .05, (NI, D)).astype(np.float32)
    uid = rng.integers(0, NU, (K, B)).astype(np.int32)
    pid = rng.integers(0, NI, (K, B)).astype(np.int32)
    nid = rng.integers(0, NI, (K, B)).astype(np.int32)
    uid[:, :2] = 7                                   # user 7 exactly twice
    uid[:, 2:14] = 3                                 # user 3 twelve times
    uid[:, 100:130] = 9; uid[:, 130:160] = 10; uid[:, 160:190] = 11      # three users 30 times: a staging plan, long segments
    # (reduction tree); lr * 30 < 2 keeps a row's own summed l2 term from diverging
    pid[:, 20:22] = 5; nid[:, 30] = 5                # item 5 three times, as positive and negative
    nid[:, 40:60] = pid[:, 40:60]                    # p == n
    uid[:, -1], pid[:, -1], nid[:, -1] = NU - 1, NI - 1, 0
    return U, V, uid, pid, nid


def _native(rt, name, lr=LR):
    if name == "sgd":
        return rt.Optimizer.sgd(lr)
    if name == "adagrad":
        return rt.Optimizer.adagrad(lr)
    if name in ("momentum", "nesterov"):
        return rt.Optimizer.momentum(lr, 0.9, name == "nesterov")
    return rt.Optimizer.adam(lr)


def _oracle(name, lr=LR):
    from oracle import numpy_oracle as orc
    if name == "sgd":
        return orc.SGD(lr)
    if name == "adagrad":
        return orc.Adagrad(lr, 0.1, 1e-7)
    if name in ("momentum", "nesterov"):
        return Momentum(lr, 0.9, name == "nesterov")
    return orc.AdamTFSparse(lr)


def _restated(U, V, uid, pid, nid, oo):
    """K steps of the biased oracle on a bias table that is zero whenever a step starts -> per-step (loss, l2)"""
    from oracle import numpy_oracle as orc
    bz = np.zeros((V.shape[0], 1), U.dtype)
    out = []
    for s in range(uid.shape[0]):
        out.append(orc.bpr_step(U, V, bz, uid[s], pid[s], nid[s], oo))
        bz[:] = 0
    return out


def _slots_of(oo, name):
    """the oracle's optimizer slots of U and V: [(slot index, U slot, V slot)]"""
    if name == "adagrad":
        return [(0, oo.acc["U"], oo.acc["V"])]
    if name in ("momentum", "nesterov"):
        return [(0, oo.vel["U"], oo.vel["V"])]
    if name == "adam":
        return [(0, oo.m["U"], oo.m["V"]), (1, oo.v["U"], oo.v["V"])]
    return []


def _check(rt, name, D, K, U, V, uid, pid, nid, lr=LR, what=""):
    B = uid.shape[1]
    U0, V0 = U.copy(), V.copy()
    tU = rt.Table(*U.shape).write(U); tV = rt.Table(*V.shape).write(V)
    opt = _native(rt, name, lr)
    loss, l2 = rt.pairwise_step("bpr", opt, tU, tV, None, uid, pid, nid, K=K, B=B)
    oo = _oracle(name, lr)
    want = _restated(U, V, uid, pid, nid, oo)
    tol = TOL_ADAM if name == "adam" else TOL
    what = f"{what} {name} D={D} K={K}"
    for s, (lr_, l2r) in enumerate(want):
        assert abs(loss[s] - lr_) <= tol * abs(lr_) and abs(l2[s] - l2r) <= tol * abs(l2r), (what, s, loss[s], lr_, l2[s], l2r)
    gU, gV = tU.read(), tV.read()
    if name == "adam":
        assert rel_err(gU, U) < TOL_ADAM and rel_err(gV, V) < TOL_ADAM, what
    else:
        delta_check(U0, gU, U, steps=K, what=what + " U")
        delta_check(V0, gV, V, steps=K, what=what + " V")
    for k, sU, sV in _slots_of(oo, name):
        assert rel_err(opt.slot(tU, k), sU) < tol and rel_err(opt.slot(tV, k), sV) < tol, (what, k)
    assert all(t is not None for t in opt._tables)
    return tU, tV, opt


@pytest.mark.parametrize("K", [1, 20])
@pytest.mark.parametrize("D", [16, 32, 50, 64, 128, 256])
@pytest.mark.parametrize("name", OPTS)
def test_training_matches_the_restatement(name, D, K):
    rt = _rt()
    U, V, uid, pid, nid = _pair_case(31 + D + K, 20000, 3000, 1024, D, K)
    _check(rt, name, D, K, U, V, uid, pid, nid, lr=0.002 if name == "adam" else LR)


@pytest.mark.parametrize("fallback", ["1", "2", "8"])
@pytest.mark.parametrize("name,D", [("sgd", 64), ("adagrad", 32), ("nesterov", 128), ("adam", 64), ("sgd", 50)])
def test_fallback_routes(fallback, name, D, monkeypatch):
    """ORX_FORCE_FALLBACK (read per call): 1 = no role bits (atomics, separate dup_apply launches), 2 = no in-launch apply,
    8 = atomics instead of staging slots"""
    monkeypatch.setenv("ORX_FORCE_FALLBACK", fallback)
    rt = _rt()
    U, V, uid, pid, nid = _pair_case(41 + D, 20000, 3000, 1024, D, 6)
    _check(rt, name, D, 6, U, V, uid, pid, nid, lr=0.002 if name == "adam" else LR, what=f"fallback={fallback}")


def _twice_case(seed, K, B, D, NU, NI):
    """every user referenced exactly twice per step, 64 items twice, the others once: no row of >= 3 references (whose fp32
    atomics would sum in a run-dependent order)"""
    rng = np.random.default_rng(seed)
    U = rng.uniform(-.05, .05, (NU, D)).astype(np.float32); V = rng.uniform(-.05, .05, (NI, D)).astype(np.float32)
    uid = np.stack([rng.permutation(np.concatenate([u, u])) for u in (rng.permutation(NU)[:B // 2] for _ in range(K))]).astype(np.int32)
    items = [rng.permutation(NI)[:2 * B - 64] for _ in range(K)]
    items = np.stack([rng.permutation(np.concatenate([it, it[:64]])) for it in items]).astype(np.int32)
    return U, V, uid, np.ascontiguousarray(items[:, :B]), np.ascontiguousarray(items[:, B:])


@pytest.mark.parametrize("D", [64, 50])
@pytest.mark.parametrize("name", ["sgd", "adagrad", "momentum", "nesterov"])
def test_bit_identical_to_the_biased_kernel_on_a_zero_bias(name, D):
    """K = 1 calls of the biased route on a bias table refilled with zeros before every call, against the bias-free route: with
    bp = bn = 0 the score x = red + bp - bn is red exactly and every row gradient takes the same operations, so U, V and the
    loss agree bit for bit (rows referenced at most twice: no run-dependent atomic summation order)"""
    rt = _rt()
    K, B = 5, 2048
    U, V, uid, pid, nid = _twice_case(7 + D, K, B, D, 4000, 8000)
    res = []
    for biased in (True, False):
        tU = rt.Table(*U.shape).write(U); tV = rt.Table(*V.shape).write(V)
        tb = rt.Table(V.shape[0], 1) if biased else None
        opt = _native(rt, name)
        losses = []
        for s in range(K):
            if biased:
                tb.fill(0.0)
            losses.append(rt.pairwise_step("bpr", opt, tU, tV, tb, uid[s], pid[s], nid[s], K=1, B=B))
        res.append((tU.read(), tV.read(), np.array(losses)))
    for a, c in zip(*res):
        assert np.array_equal(a, c), (name, D)


def test_lazy_adam_equals_dense_adam_and_resumes_from_a_checkpoint(monkeypatch):
    """lazy Adam (rows replay their gradient-free steps when next referenced, a read flushes) against ORX_ADAM_DENSE=1 (every
    reference accumulates, whole-table sweeps); then a save / load round trip of [U, V] with the optimizer resumes: the same losses
    bit for bit, the same tables to TOL"""
    rt = _rt()
    D, K, B, calls = 64, 4, 1024, 3
    U, V, uid, pid, nid = _pair_case(5, 20000, 3000, B, D, K * calls * 2)
    out = {}
    for dense in (False, True):
        if dense:
            monkeypatch.setenv("ORX_ADAM_DENSE", "1")
        else:
            monkeypatch.delenv("ORX_ADAM_DENSE", raising=False)
        tU = rt.Table(*U.shape).write(U); tV = rt.Table(*V.shape).write(V)
        opt = rt.Optimizer.adam(0.002)
        for c in range(calls):
            sl = slice(c * K, (c + 1) * K)
            rt.pairwise_step("bpr", opt, tU, tV, None, uid[sl], pid[sl], nid[sl], K=K, B=B, want_loss=False)
        out[dense] = (tU.read(), tV.read(), opt.slot(tU, 0), opt.slot(tV, 1))
        if not dense:
            lazy = (tU, tV, opt)
    for a, c in zip(out[False], out[True]):
        assert rel_err(a, c) < TOL_ADAM
    monkeypatch.delenv("ORX_ADAM_DENSE", raising=False)
    tU, tV, opt = lazy
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "nobias.npz")
        rt.save_checkpoint(path, {"U": tU, "V": tV}, opt)
        rU = rt.Table(*U.shape); rV = rt.Table(*V.shape); ropt = rt.Optimizer.adam(0.002)
        rt.load_checkpoint(path, {"U": rU, "V": rV}, ropt)
    assert ropt.step == opt.step
    for c in range(calls, 2 * calls):
        sl = slice(c * K, (c + 1) * K)
        la = rt.pairwise_step("bpr", opt, tU, tV, None, uid[sl], pid[sl], nid[sl], K=K, B=B)
        lb = rt.pairwise_step("bpr", ropt, rU, rV, None, uid[sl], pid[sl], nid[sl], K=K, B=B)
        assert np.array_equal(la[0], lb[0])
    # (the rows a read flushes replay their gradient-free steps in closed form from a table of per-step moments that each optimizer
    # object builds for its own horizon: the last bits of a replayed row may differ, the losses above may not)
    for a, c in ((tU.read(), rU.read()), (tV.read(), rV.read()), (opt.slot(tU, 0), ropt.slot(rU, 0)), (opt.slot(tV, 1), ropt.slot(rV, 1))):
        assert rel_err(a, c) < TOL


def test_full_size_c2_matches_the_c_oracle():
    """C2's shape (BPR D = 64, 1M x 1M, B = 65 536) in bench's form: device ids, one K = 20 call with no loss read-back, the
    tables read at the end; against the C oracle with its bias table re-zeroed before every step"""
    import torch
    from oracle import c_oracle
    rt = _rt()
    NU = NI = 1_000_000
    B, K, D = 65536, 20, 64
    rng = np.random.default_rng(12)
    U = rng.uniform(-.05, .05, (NU, D)).astype(np.float32); V = rng.uniform(-.05, .05, (NI, D)).astype(np.float32)
    uid = rng.integers(0, NU, (K, B)).astype(np.int32); pid = rng.integers(0, NI, (K, B)).astype(np.int32)
    nid = rng.integers(0, NI, (K, B)).astype(np.int32)
    tU = rt.Table(NU, D).write(U); tV = rt.Table(NI, D).write(V)
    opt = rt.Optimizer.sgd(0.05)
    dev = [torch.from_numpy(x).cuda() for x in (uid, pid, nid)]
    U0, V0 = U.copy(), V.copy()
    rt.pairwise_step("bpr", opt, tU, tV, None, *dev, K=K, B=B, want_loss=False)
    gU, gV = tU.read(), tV.read()
    bz = np.zeros((NI, 1), np.float32)
    cpu = c_oracle.PairwiseCPU("bpr", "sgd", U, V, bz, lr=0.05)
    for s in range(K):
        cpu.step(uid[s], pid[s], nid[s])
        bz[:] = 0
    for nm, w0, got, want in (("user", U0, gU, U), ("item", V0, gV, V)):
        coef = delta_check(w0, got, want, steps=K, what=f"bias-free C2 {nm}")
        assert abs(coef - 1.0) <= 1e-4, (nm, coef)
    untouched_u = np.ones(NU, bool); untouched_u[uid.reshape(-1)] = False
    untouched_i = np.ones(NI, bool); untouched_i[pid.reshape(-1)] = False; untouched_i[nid.reshape(-1)] = False
    assert untouched_u.sum() > 0.1 * NU and untouched_i.sum() > 0.05 * NI
    assert np.array_equal(gU[untouched_u], U0[untouched_u]) and np.array_equal(gV[untouched_i], V0[untouched_i])


@pytest.mark.parametrize("D", [64, 50])
def test_forward_loss_matches_the_restatement(D):
    from oracle import numpy_oracle as orc
    rt = _rt()
    U, V, uid, pid, nid = _pair_case(3, 20000, 3000, 1024, D, 1)
    tU = rt.Table(*U.shape).write(U); tV = rt.Table(*V.shape).write(V)
    loss, l2 = rt.pairwise_loss("bpr", tU, tV, None, uid[0], pid[0], nid[0])
    lr_, l2r, _ = orc.bpr_forward(U, V, np.zeros((V.shape[0], 1), np.float32), uid[0], pid[0], nid[0])
    assert abs(loss - lr_) <= TOL * abs(lr_) and abs(l2 - l2r) <= TOL * abs(l2r)
    assert np.array_equal(tU.read(), U) and np.array_equal(tV.read(), V)


@pytest.mark.parametrize("D", [64, 50])
def test_hogwild_on_unique_ids_equals_the_exact_step(D):
    rt = _rt()
    rng = np.random.default_rng(8)
    B = 1024
    U = rng.uniform(-.05, .05, (4000, D)).astype(np.float32); V = rng.uniform(-.05, .05, (5000, D)).astype(np.float32)
    uid = rng.permutation(4000)[:B].astype(np.int32)
    items = rng.permutation(5000)[:2 * B].astype(np.int32)
    pid, nid = items[:B].copy(), items[B:].copy()
    res = []
    for hogwild in (False, True):
        tU = rt.Table(*U.shape).write(U); tV = rt.Table(*V.shape).write(V)
        loss, l2 = rt.pairwise_step("bpr", rt.Optimizer.sgd(LR), tU, tV, None, uid, pid, nid, hogwild=hogwild)
        res.append((tU.read(), tV.read(), loss, l2))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert abs(res[0][2][0] - res[1][2][0]) <= TOL * abs(res[0][2][0])


def _nobias_fixtures():
    from conftest import GOLDEN
    import glob
    return sorted(glob.glob(os.path.join(GOLDEN, "refstub", "bprnb_*.npz")))


@pytest.mark.parametrize("path", _nobias_fixtures(), ids=os.path.basename)
def test_reference_fixtures_on_the_device(path):
    """tests/golden/refstub/bprnb_*.npz (the reference's LatentFactor and PairwiseLogLoss in a bias-free model, minted by
    tests/golden/make_golden_nobias.py) fed to the device path, step by step"""
    from conftest import OPT_KW
    rt = _rt()
    z = np.load(path)
    opt_name = os.path.basename(path).split("_")[2]
    tU = rt.Table(*z["in_U"].shape).write(z["in_U"].astype(np.float32)); tV = rt.Table(*z["in_V"].shape).write(z["in_V"].astype(np.float32))
    kw = dict(OPT_KW[opt_name])
    lr = kw.pop("lr")
    opt = {"sgd": rt.Optimizer.sgd, "adagrad": rt.Optimizer.adagrad, "adam": rt.Optimizer.adam}[opt_name](lr, **kw)
    tol = TOL_ADAM if opt_name == "adam" else TOL
    for s in range(int(z["steps"])):
        uid, pid, nid = np.roll(z["in_uid"], s), np.roll(z["in_pid"], 2 * s), np.roll(z["in_nid"], 3 * s)
        loss, l2 = rt.pairwise_step("bpr", opt, tU, tV, None, uid, pid, nid)
        want_loss, want_l2 = z["losses"][s]
        assert abs(loss[0] - want_loss) <= tol * abs(want_loss) and abs(l2[0] - want_l2) <= tol * abs(want_l2), s
    assert rel_err(tU.read(), z["out_U"]) < tol and rel_err(tV.read(), z["out_V"]) < tol


# ---- the packaged BPR without item biases ---------------------------------------------------------------------------------
def _model(NU, NI, D):
    from openrec_amd.tf2.recommenders import BPR
    m = BPR(dim_user_embed=D, dim_item_embed=D, total_users=NU, total_items=NI, use_item_bias=False)
    assert m.item_bias is None and len(m.trainable_variables) == 2
    return m


@pytest.mark.parametrize("optname", ["sgd", "adam"])
def test_bpr_without_item_bias_trains_under_a_tape(optname):
    from openrec_amd.tf2 import compat
    compat.install()
    import tensorflow as tf
    NU, NI, D, B = 700, 900, 32, 1024
    model = _model(NU, NI, D)
    opt = tf.keras.optimizers.SGD(0.05) if optname == "sgd" else tf.keras.optimizers.Adam(0.002)

    def train_step(*batch):
        with tf.GradientTape() as tape:
            loss_value = model(*batch)
        gradients = tape.gradient(loss_value, model.trainable_variables)
        opt.apply_gradients(zip(gradients, model.trainable_variables))
        return loss_value

    U, V = (np.array(v.numpy()) for v in model.trainable_variables)
    U0, V0 = U.copy(), V.copy()
    oo = _oracle(optname, 0.05 if optname == "sgd" else 0.002)
    rng = np.random.default_rng(5)
    ids = [tuple(rng.integers(0, hi, B).astype(np.int32) for hi in (NU, NI, NI)) for _ in range(4)]
    out = [train_step(*b) for b in ids]
    want = _restated(U, V, *(np.stack([b[k] for b in ids]) for k in range(3)), oo)
    tol = TOL_ADAM if optname == "adam" else TOL
    for (loss, l2), (lr_, l2r) in zip(out, want):
        assert abs(float(loss) - lr_) <= tol * abs(lr_) and abs(float(l2) - l2r) <= tol * abs(l2r)
    # outside a tape: the forward alone, on the device, tables untouched
    loss_f, l2_f = model(*ids[0])
    got = [np.asarray(v.numpy()) for v in model.trainable_variables]
    for nm, w0, g, w in zip("UV", (U0, V0), got, (U, V)):
        if optname == "adam":
            assert rel_err(g.reshape(w.shape), w) < TOL_ADAM, nm
        else:
            delta_check(w0, g.reshape(w.shape), w, steps=4, what=f"BPR(use_item_bias=False) {nm}")
    from oracle import numpy_oracle as orc
    lr_, l2r, _ = orc.bpr_forward(got[0], got[1], np.zeros((NI, 1), np.float32), *ids[0])
    assert abs(float(loss_f) - lr_) <= TOL * abs(lr_) and abs(float(l2_f) - l2r) <= TOL * abs(l2r)


def test_bpr_without_item_bias_train_steps_inference_evaluate():
    from oracle import metrics_oracle as mo
    rt = _rt()
    NU, NI, D, B, K = 500, 700, 64, 512, 3
    model = _model(NU, NI, D)
    U, V = (np.array(v.numpy()) for v in model.trainable_variables)
    rng = np.random.default_rng(9)
    uid, pid, nid = (rng.integers(0, hi, (K, B)).astype(np.int32) for hi in (NU, NI, NI))
    loss, l2 = model.train_steps(rt.Optimizer.sgd(LR), uid, pid, nid)
    U0, V0 = U.copy(), V.copy()
    want = _restated(U, V, uid, pid, nid, _oracle("sgd"))
    for s, (lr_, l2r) in enumerate(want):
        assert abs(loss[s] - lr_) <= TOL * abs(lr_)
    gU, gV = (np.asarray(v.numpy()).reshape(w.shape) for v, w in zip(model.trainable_variables, (U, V)))
    delta_check(U0, gU, U, steps=K, what="train_steps U"); delta_check(V0, gV, V, steps=K, what="train_steps V")
    q = np.array([0, 3, NU - 1, 17], np.int32)
    scores = np.asarray(model.inference(q))
    ref = gU[q].astype(np.float64) @ gV.T.astype(np.float64)
    assert scores.shape == (q.size, NI) and np.abs(scores - ref).max() <= 1e-5 * np.abs(ref).max()
    pos = np.zeros((q.size, NI), bool); excl = np.zeros((q.size, NI), bool)
    for r in range(q.size):
        pos[r, rng.choice(NI, 20, replace=False)] = True
        excl[r, rng.choice(NI, 10, replace=False)] = True
    excl &= ~pos
    pred = scores.astype(np.float32)          # (the metrics rank the device's scores: ties of a host matmul could rank otherwise)
    for masks in ((pos, excl), (rt.SparseMask.from_dense(pos), rt.SparseMask.from_dense(excl))):
        res = model.evaluate(q, *masks, at=[10, 50])
        assert np.allclose(res["auc"], mo.auc(pos, pred, excl), rtol=1e-5, atol=1e-6)
        assert np.allclose(np.asarray(res["ndcg"]).reshape(q.size, -1), mo.ndcg(pos, pred, excl, at=[10, 50]), rtol=1e-5, atol=1e-6)
        assert np.allclose(np.asarray(res["recall"]).reshape(q.size, -1), mo.recall(pos, pred, excl, at=[10, 50]), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("D", [64, 300])
def test_score_all_items_without_bias(D):
    """both scorers: the matrix-core one (D <= 256) and the plain one (larger D); host and device output"""
    rt = _rt()
    rng = np.random.default_rng(D)
    U = rng.uniform(-.05, .05, (300, D)).astype(np.float32); V = rng.uniform(-.05, .05, (1001, D)).astype(np.float32)
    tU = rt.Table(*U.shape).write(U); tV = rt.Table(*V.shape).write(V)
    q = np.array([1, 0, 299, 5, 5], np.int32)
    ref = U[q].astype(np.float64) @ V.T.astype(np.float64)
    for kind, want in (("dot", ref), ("l2", -((U[q, None, :].astype(np.float64) - V[None]) ** 2).sum(-1))):
        for device in (False, True):
            got = np.asarray(rt.score_all_items(kind, tU, tV, None, q, device=device))
            assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), (kind, device)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def _tables(rt, D=64):
    return rt.Table(100, D).init_uniform(), rt.Table(200, D).init_uniform()


def test_ucml_and_censor_refuse_a_missing_bias():
    rt = _rt()
    tU, tV = _tables(rt)
    ids = np.zeros(8, np.int32)
    with pytest.raises(ValueError, match="bias"):
        rt.pairwise_step("ucml", rt.Optimizer.sgd(LR), tU, tV, None, ids, ids, ids)
    with pytest.raises(ValueError, match="bias"):
        rt.pairwise_loss("ucml", tU, tV, None, ids, ids, ids)
    with pytest.raises(ValueError, match="bias"):
        rt.pairwise_step("bpr", rt.Optimizer.sgd(LR), tU, tV, None, ids, ids, ids, censor=True)


def test_sharded_entry_points_refuse_a_missing_bias():
    import ctypes
    from openrec_amd import _ffi
    from openrec_amd.sharded import HipBackend
    rt = _rt()
    tU, tV = _tables(rt)
    opt = rt.Optimizer.sgd(LR)
    lib = tU.ctx._lib
    n = ctypes.c_void_p()
    for fn, extra in ((lib.orx_sharded_pairwise_steps, ()), (lib.orx_sharded_pairwise_steps_hot, (None, None, 0, 1.0))):
        rc = fn(None, opt._h, _ffi.ORX_BPR, tU._h, tV._h, None, *extra, None, None, None, 1, 8, 8, 100, 200, 0.5, 1.5, 1, 0, None, None)
        assert rc == _ffi.ORX_ERR_ARG
        with pytest.raises(ValueError, match="bias"):
            _ffi.check(rc)
    with pytest.raises(ValueError, match="bias"):
        HipBackend.sharded_steps(None, n, "bpr", tU, tV, None, None, None, None, 100, 200, 0.5, 1.5, 1, False, None, None)
