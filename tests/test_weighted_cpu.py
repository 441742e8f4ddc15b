"""The weighted objective (per-triplet weights, l2 coefficient) as far as it can be checked without a device:

* tests/weighted_ref.py -- the expectation of tests/test_gpu_weighted.py, composed from the unchanged oracle -- against fixtures
  minted from the reference's own class text with the target `loss + 0.01 * l2_loss` (tests/golden/make_golden_l2reg.py), at
  the bounds of tests/test_reference_goldens.py; its exact equality with the oracle's step at w = 1, l2_reg = 1; the replication
  property of integer weights; an independent torch-autograd restatement of the weighted losses;
* the boundary: the new entry points are declared, exported and typed, and the runtime refuses bad combinations before any
  device call; the step queue keeps weighted and unweighted steps apart."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, OPT_KW, ROOT, rel_err
from oracle import numpy_oracle as orc
import weighted_ref as wr

REFSTUB = os.path.join(GOLDEN, "refstub")


def _reg_fixtures():
    return sorted(f for f in os.listdir(REFSTUB) if re.match(r"(bpr|ucml|wrmf|gmf)reg_", f) and f.endswith(".npz")) if os.path.isdir(REFSTUB) else []


def _opt(kind):
    return {"sgd": orc.SGD, "adagrad": orc.Adagrad, "adam": orc.AdamTFSparse}[kind](**OPT_KW[kind])


def _slots(oo, kind):
    return {"sgd": {}, "adagrad": {"acc": getattr(oo, "acc", None)}, "adam": {"m": getattr(oo, "m", None), "v": getattr(oo, "v", None)}}[kind]


def test_the_l2reg_fixtures_are_there():
    names = _reg_fixtures()
    assert 8 <= len(names) <= 12 and {n.split("reg_")[0] for n in names} == {"bpr", "ucml", "wrmf", "gmf"}


@pytest.mark.parametrize("dtype,tol", [(np.float64, 2e-7), (np.float32, 1e-5)])
@pytest.mark.parametrize("fname", _reg_fixtures())
def test_weighted_ref_matches_the_reference_text_with_an_l2_coefficient(fname, dtype, tol):
    """the reference's BPR / UCML / WRMF / GMF trained on `loss + 0.01 * l2_loss`: weighted_ref at l2_reg = 0.01 (no weights) gives
    the same losses (l2 unscaled), tables and slots.  Bounds as tests/test_reference_goldens.py: 2e-7 in float64 (the files store
    float32), 1e-5 in float32."""
    g = dict(np.load(os.path.join(REFSTUB, fname)))
    model, _, optkind, _ = fname[:-4].split("_")
    model = model[:-3]
    l2_reg = float(g["l2_reg"])
    assert l2_reg == 0.01
    W = {k: g["in_" + k].astype(dtype) for k in ("U", "V", "b")}
    if model == "gmf":
        W["w"] = g["in_w"].astype(dtype)
    oo = _opt(optkind)
    losses = []
    for s in range(int(g["steps"])):
        uid, pid = np.roll(g["in_uid"], s), np.roll(g["in_pid"], 2 * s)
        if model in ("wrmf", "gmf"):
            lab = np.roll(g["in_label"], s).astype(dtype)
            losses.append(wr.point_step(model, W["U"], W["V"], W["b"], W.get("w"), uid, pid, lab, oo, l2_reg=l2_reg, a=2.0, b_w=0.5))
        else:
            losses.append(wr.pair_step(model, W["U"], W["V"], W["b"], uid, pid, np.roll(g["in_nid"], 3 * s), oo, l2_reg=l2_reg))
    assert rel_err(np.array(losses, np.float64), g["losses"]) < tol
    for k in W:
        assert rel_err(W[k], g["out_" + k]) < tol, k
        for short, store in _slots(oo, optkind).items():
            assert rel_err(store[k], g["slot_%s_%s" % (k, short)]) < tol, (k, short)


def _inputs(seed=3, NU=40, NI=60, B=96, D=8, dtype=np.float64):
    rng = np.random.default_rng(seed)
    U = rng.uniform(-.5, .5, (NU, D)).astype(dtype); V = rng.uniform(-.5, .5, (NI, D)).astype(dtype); b = rng.uniform(-.5, .5, (NI, 1)).astype(dtype)
    uid = rng.integers(0, NU, B).astype(np.int32); pid = rng.integers(0, NI, B).astype(np.int32); nid = rng.integers(0, NI, B).astype(np.int32)
    return U, V, b, uid, pid, nid, rng


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("optkind", ["sgd", "adagrad", "adam"])
@pytest.mark.parametrize("model", ["bpr", "ucml", "wrmf", "gmf"])
def test_unit_weights_and_coefficient_one_are_the_oracle_step_exactly(model, optkind, dtype):
    U, V, b, uid, pid, nid, rng = _inputs(dtype=dtype)
    lab = (rng.random(uid.size) < 0.4).astype(dtype)
    wd = rng.uniform(-.3, .3, (U.shape[1], 1)).astype(dtype)
    A = [x.copy() for x in (U, V, b, wd)]; Bv = [x.copy() for x in (U, V, b, wd)]
    oa, ob = _opt(optkind), _opt(optkind)
    for s in range(2):
        u_, p_, n_ = np.roll(uid, s), np.roll(pid, 2 * s), np.roll(nid, 3 * s)
        if model == "bpr":
            want = orc.bpr_step(A[0], A[1], A[2], u_, p_, n_, oa)
            got = wr.pair_step("bpr", Bv[0], Bv[1], Bv[2], u_, p_, n_, ob, w=np.ones(uid.size, dtype), l2_reg=1.0)
        elif model == "ucml":
            want = orc.ucml_step(A[0], A[1], A[2], u_, p_, n_, oa, margin=0.5, do_censor=True)
            got = wr.pair_step("ucml", Bv[0], Bv[1], Bv[2], u_, p_, n_, ob, w=np.ones(uid.size, dtype), l2_reg=1.0, censor=True)
        elif model == "wrmf":
            want = orc.wrmf_step(A[0], A[1], A[2], u_, p_, lab, oa, a=2.0, b_w=0.5)
            got = wr.point_step("wrmf", Bv[0], Bv[1], Bv[2], None, u_, p_, lab, ob, l2_reg=1.0, a=2.0, b_w=0.5)
        else:
            want = orc.gmf_step(A[0], A[1], A[2], A[3], u_, p_, lab, oa)
            got = wr.point_step("gmf", Bv[0], Bv[1], Bv[2], Bv[3], u_, p_, lab, ob, l2_reg=1.0)
        assert tuple(want) == tuple(got)
    for x, y in zip(A, Bv):
        assert np.array_equal(x, y)
    for short, store in _slots(oa, optkind).items():
        for k in store:
            assert np.array_equal(store[k], _slots(ob, optkind)[short][k]), (short, k)


@pytest.mark.parametrize("model", ["bpr", "ucml"])
def test_the_two_forms_of_the_weighted_gradient_agree(model):
    """(w g) A + l2_reg row, as weighted_ref forms it, against w (g_full - row) + l2_reg row, as the objective is usually stated"""
    U, V, b, uid, pid, nid, rng = _inputs()
    w = rng.uniform(0, 2, uid.size)
    a = wr.pair_grads(model, U, V, b, uid, pid, nid, w, 0.01)
    d = wr.pair_grads_by_difference(model, U, V, b, uid, pid, nid, w, 0.01)
    for k in a:
        assert np.abs(a[k] - d[k]).max() <= 1e-12 * max(np.abs(d[k]).max(), 1.0), k


@pytest.mark.parametrize("model", ["bpr", "ucml"])
def test_integer_weights_are_repeated_triplets(model):
    """float64, l2_reg = 0, SGD: weights in {0, 1, 2, 3} give the tables of the oracle's UNWEIGHTED loss gradient (its coefficient
    `g` on the pre-step tables, its SGD) on the batch with triplet i repeated w_i times -- BPR's loss is a mean over the batch, so
    the repeated batch of B' triplets takes lr * B' / B; UCML's is a sum and keeps lr."""
    U, V, b, uid, pid, nid, rng = _inputs(seed=5)
    w = rng.integers(0, 4, uid.size)
    assert set(w) == {0, 1, 2, 3}
    lr = 0.05
    Uw, Vw, bw = U.copy(), V.copy(), b.copy()
    loss_w, _ = wr.pair_step(model, Uw, Vw, bw, uid, pid, nid, orc.SGD(lr=lr), w=w.astype(np.float64), l2_reg=0.0)
    ru, rp, rn = (np.repeat(x, w) for x in (uid, pid, nid))
    Bw, Bp = uid.size, ru.size
    Ur, Vr, br = U.copy(), V.copy(), b.copy()
    if model == "bpr":
        loss_r, _, _ = orc.bpr_forward(U, V, b, ru, rp, rn)
        g = orc.bpr_grads(U, V, b, ru, rp, rn)["g"]
        gu, gp, gn, gbp, gbn = g[:, None] * (V[rp] - V[rn]), g[:, None] * U[ru], -g[:, None] * U[ru], g, -g
        oo = orc.SGD(lr=lr * Bp / Bw)
        loss_r = loss_r * Bp / Bw
    else:
        loss_r, _, _ = orc.ucml_forward(U, V, b, ru, rp, rn, 0.5)
        a = orc.ucml_grads(U, V, b, ru, rp, rn, 0.5)["g"]
        gu, gp, gn, gbp, gbn = -2 * a[:, None] * (V[rp] - V[rn]), -2 * a[:, None] * (U[ru] - V[rp]), 2 * a[:, None] * (U[ru] - V[rn]), -a, a
        oo = orc.SGD(lr=lr)
    oo.apply(Ur, ru, gu, key="U")
    oo.apply(Vr, np.concatenate([rp, rn]), np.concatenate([gp, gn]), key="V")
    oo.apply(br, np.concatenate([rp, rn]), np.concatenate([gbp, gbn])[:, None], key="b")
    assert abs(loss_w - loss_r) <= 1e-12 * abs(loss_r)
    for got, want in ((Uw, Ur), (Vw, Vr), (bw, br)):
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert not np.array_equal(Uw, U)


@pytest.mark.parametrize("model", ["bpr", "ucml"])
def test_torch_autograd_restatement_of_the_weighted_loss(model):
    """J = loss_w + l2_reg * l2_loss written once more with torch (float64) on the gathered rows: the same per-occurrence gradients"""
    import torch
    U, V, b, uid, pid, nid, rng = _inputs(seed=7)
    w = rng.uniform(0, 2, uid.size); w[::9] = 0.0
    l2_reg, margin = 0.01, 0.5
    t = lambda x: torch.tensor(x, dtype=torch.float64, requires_grad=True)
    u, p, n, bp, bn = t(U[uid]), t(V[pid]), t(V[nid]), t(b[pid, 0]), t(b[nid, 0])
    tw = torch.tensor(w, dtype=torch.float64)
    if model == "bpr":
        x = (u * p).sum(1) + bp - ((u * n).sum(1) + bn)
        loss = (tw * -torch.nn.functional.logsigmoid(torch.clamp(x, min=-30.0))).mean()
    else:
        diff = (-((u - p) ** 2).sum(1) + bp) - (-((u - n) ** 2).sum(1) + bn)
        loss = (tw * torch.clamp(margin - diff, min=0.0)).sum()
    l2 = ((u * u).sum() + (p * p).sum() + (n * n).sum()) / 2
    (loss + l2_reg * l2).backward()
    got = wr.pair_grads(model, U, V, b, uid, pid, nid, w, l2_reg, margin)
    want = dict(gu=u.grad, gp=p.grad, gn=n.grad, gbp=bp.grad, gbn=bn.grad)
    for k, v in want.items():
        v = v.numpy()
        assert np.abs(got[k] - v).max() <= 1e-12 * max(np.abs(v).max(), 1.0), k
    lw, l2w = wr.pair_forward(model, U, V, b, uid, pid, nid, w, margin)
    assert abs(lw - loss.item()) <= 1e-12 * abs(loss.item()) and abs(l2w - l2.item()) <= 1e-12 * l2.item()


# ---- the boundary -------------------------------------------------------------------------------------------------------------
def _decl_args(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "openrec_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S)
    assert m, f"{name} is not declared in openrec_hip.h"
    return [a.strip() for a in m.group(1).split(",") if a.strip()]


@pytest.mark.parametrize("name,base,extra", [("orx_pairwise_step_weighted", "orx_pairwise_step_subset", 2), ("orx_pairwise_loss_weighted", "orx_pairwise_loss", 1),
                                             ("orx_pointwise_step_l2reg", "orx_pointwise_step_subset", 1),
                                             ("orx_sampler_set_record_weights", None, 0), ("orx_sampler_pairwise_weights", None, 0)])
def test_entry_points_are_declared_exported_and_typed(name, base, extra):
    from openrec_amd import _ffi
    lib = _ffi.load()
    assert hasattr(lib, name)
    res, args = _ffi.SIGNATURES[name]
    assert res is _ffi.c_int and len(args) == len(_decl_args(name))
    if base:
        assert len(args) == len(_ffi.SIGNATURES[base][1]) + extra
    floats = [i for i, a in enumerate(_decl_args(name)) if re.match(r"float\s+\w+$", a)]
    assert all(args[i] is _ffi.c_float for i in floats) and sum(a is _ffi.c_float for a in args) == len(floats)


from runtime_standin import NoDevice as _NoDevice


class _FakeDeviceTensor:
    is_cuda = True
    dtype = "torch.float32"

    def __init__(self, n):
        self._n = n

    def data_ptr(self):
        return 0x1000

    def numel(self):
        return self._n

    def is_contiguous(self):
        return True


def test_runtime_refuses_before_any_device_call():
    from openrec_amd import runtime as rt
    t = _NoDevice()
    ids = np.zeros(4, np.int32)
    with pytest.raises(ValueError, match="no_l2"):
        rt.pairwise_step("bpr", t, t, t, t, ids, ids, ids, no_l2=True, l2_reg=0.01)
    with pytest.raises(ValueError, match="no_l2"):
        rt.pointwise_step("wrmf", t, t, t, t, None, ids, ids, ids.astype(np.float32), no_l2=True, l2_reg=0.01)

    class _Ctx:
        _lib = None

        def after_torch(self, *a):
            pass

    class _T:
        ctx = _Ctx()
    with pytest.raises(ValueError, match="weights on the device with ids on the host"):
        rt.pairwise_step("bpr", t, _T(), t, t, ids, ids, ids, weights=_FakeDeviceTensor(4))
    with pytest.raises(ValueError, match="3 weights for 4 ids"):
        rt.pairwise_step("bpr", t, _T(), t, t, ids, ids, ids, weights=np.ones(3, np.float32))
    with pytest.raises(ValueError, match="weights on the device with ids on the host"):
        rt.pairwise_loss("bpr", _T(), t, t, ids, ids, ids, weights=_FakeDeviceTensor(4))


def test_recommenders_take_an_l2_coefficient():
    import inspect
    from openrec_amd.tf2.recommenders import BPR, GMF, UCML, WRMF
    from openrec_amd.tf2.recommenders._base import Recommender
    for cls in (BPR, UCML, GMF, WRMF):
        assert inspect.signature(cls.__init__).parameters["l2_reg"].default == 1.0
    m = Recommender.__new__(Recommender)
    assert m.l2_reg == 1.0 and m._l2_arg(False) is None and m._l2_arg(True) is None      # the reference: today's entry points
    m._set_l2_reg(0.01)
    assert m._l2_arg(False) == 0.01 and m._l2_arg(True) is None
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="l2_reg"):
            m._set_l2_reg(bad)


def test_lazy_second_output_is_scaled_by_the_coefficient():
    from openrec_amd.tf2._lazy import LazyScalar

    class _Step:
        def forward(self):
            return (0.25, 3.0)
    assert LazyScalar(_Step(), 1).numpy() == np.float32(3.0) and LazyScalar(_Step(), 0, scale=1.0).numpy() == np.float32(0.25)
    assert LazyScalar(_Step(), 1, scale=0.01).numpy() == np.float32(3.0) * np.float32(0.01)


def test_step_queue_carries_the_weights_as_a_fourth_buffer():
    from openrec_amd.tf2.recommenders._base import _StepQueue

    class _S:
        values = None
    q = _StepQueue()
    ids = np.arange(4, dtype=np.int32)
    seen = []

    def runner(bufs, K, censor=False):
        seen.append([np.array(x) for x in bufs])
        return np.zeros(K), np.zeros(K)
    q.add(_S(), ("pair", 0.01, True), (ids, ids + 1, ids + 2, np.full(4, 0.5, np.float32)), runner)
    q.add(_S(), ("pair", 0.01, True), (ids, ids + 1, ids + 2, np.full(4, 1.5, np.float32)), runner)
    assert len(q.bufs) == 4 and q.bufs[3].dtype == np.float32
    assert q.mark_censor((ids, ids + 1, ids + 2))          # (the censor fold-in compares the three id buffers only)
    q.run()
    assert len(seen) == 2 and seen[0][3].shape == (1, 4)      # (the censored step runs as its own call)
    assert np.array_equal(seen[0][3][0], np.full(4, 0.5, np.float32)) and np.array_equal(seen[1][3][0], np.full(4, 1.5, np.float32))
