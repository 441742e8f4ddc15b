"""CPU: the reference of the N-negative step (tests/multineg_ref.py) against torch autograd and the oracle's BPR, the headroom of
the GPU tests' bounds on the shared case list (tests/multineg_cases.py), and the declarations of the three entry points."""
import os
import re

import numpy as np
import pytest

import multineg_cases as mc
import multineg_ref as mr
from conftest import ROOT, delta_check
from oracle import numpy_oracle as orc


def _small(seed, B=9, N=4, D=6, NU=5, NI=7):
    rng = np.random.default_rng(seed)
    U = rng.uniform(-1, 1, (NU, D)); V = rng.uniform(-1, 1, (NI, D)); b = rng.uniform(-1, 1, (NI, 1))
    uid = rng.integers(0, NU, B); pid = rng.integers(0, NI, B); nid = rng.integers(0, NI, (B, N))
    nid[0, 1] = nid[0, 0]                       # a negative repeated inside a sample
    nid[1, 2] = pid[1]                          # a negative equal to the positive
    w = rng.uniform(0, 2, B); w[3] = 0.0
    off = rng.normal(0, 1, (B, N)); off[2, 1] = -np.inf
    return U, V, b, uid, pid, nid, w, off


def _torch_objective(kind, U, V, b, uid, pid, nid, w, off, l2_reg):
    """J by torch in float64 on the GATHERED rows (leaves), so that autograd returns per-occurrence gradients"""
    import torch
    t = lambda x: torch.tensor(np.asarray(x, np.float64))
    u = t(U[uid]).requires_grad_(); p = t(V[pid]).requires_grad_(); n = t(V[nid]).requires_grad_()
    bp = t(b[pid, 0]).requires_grad_(); bn = t(b[nid, 0]).requires_grad_()
    sp = (u * p).sum(1) + bp
    s = (u[:, None, :] * n).sum(2) + bn + t(off)
    if kind == "softmax":
        l = torch.logsumexp(torch.cat([sp[:, None], s], 1), 1) - sp
    else:
        x = torch.maximum(sp[:, None] - s, torch.tensor(-30.0, dtype=torch.float64))
        l = (-torch.nn.functional.logsigmoid(x)).mean(1)
    loss = (t(w) * l).sum() / len(uid)
    l2 = 0.5 * ((u * u).sum() + (p * p).sum() + (n * n).sum())
    (loss + l2_reg * l2).backward()
    return float(loss.detach()), float(l2.detach()), dict(gu=u.grad.numpy(), gp=p.grad.numpy(), gn=n.grad.numpy(), gbp=bp.grad.numpy(), gbn=bn.grad.numpy())


@pytest.mark.parametrize("kind", mr.KINDS)
def test_reference_gradients_equal_torch_autograd_in_float64(kind):
    """weights (one of them 0), offsets (one of them -inf), l2_reg != 1, a repeated negative, a negative equal to the positive"""
    U, V, b, uid, pid, nid, w, off = _small(3)
    loss, l2 = mr.forward(kind, U, V, b, uid, pid, nid, w, off)
    g = mr.grads(kind, U, V, b, uid, pid, nid, w, off, l2_reg=0.3)
    tl, tl2, tg = _torch_objective(kind, U, V, b, uid, pid, nid, w, off, 0.3)
    assert abs(loss - tl) <= 1e-14 * abs(tl) and abs(l2 - tl2) <= 1e-14 * tl2
    for k in ("gu", "gp", "gn", "gbp", "gbn"):
        assert np.isfinite(g[k]).all()
        assert np.abs(g[k] - tg[k]).max() <= 1e-14, k
    assert g["gbn"][2, 1] == 0.0                # the -inf offset removes the negative


def test_the_clamp_of_the_log_sigmoid_form_routes_no_gradient():
    """s_p - s_j < -30: the term is -log_sigmoid(-30) and the negative's coefficient is 0 (Maximum sends the gradient to its
    first argument on >= only), as in the oracle's BPR"""
    U, V, b, uid, pid, nid, w, off = _small(4)
    off[:] = 0.0; off[5, 0] = 100.0
    g = mr.grads("logsig", U, V, b, uid, pid, nid, w, off)
    assert g["gbn"][5, 0] == 0.0 and (g["gbn"][5, 1:] > 0).all()
    _, _, tg = _torch_objective("logsig", U, V, b, uid, pid, nid, w, off, 1.0)
    assert np.abs(g["gbn"] - tg["gbn"]).max() <= 1e-14


def test_one_negative_is_the_oracles_bpr():
    rng = np.random.default_rng(5)
    B, D, NU, NI = 40, 8, 11, 13
    U = rng.uniform(-1, 1, (NU, D)); V = rng.uniform(-1, 1, (NI, D)); b = rng.uniform(-1, 1, (NI, 1))
    uid = rng.integers(0, NU, B); pid = rng.integers(0, NI, B); nid = rng.integers(0, NI, B)
    uid[:2] = 0; pid[:2] = (0, 1); nid[:2] = (1, 0)                    # x[1] = -x[0] ...
    U[0] *= 40.0                                                       # ... one far below the clamp, one far above
    want_loss, want_l2, x = orc.bpr_forward(U, V, b, uid, pid, nid)
    want = orc.bpr_grads(U, V, b, uid, pid, nid)
    assert (x < -30).any() and (x > 30).any()
    for kind in mr.KINDS:
        keep = np.ones(B, bool) if kind == "logsig" else x >= -30          # softmax has no clamp: equal where x >= -30
        loss, l2 = mr.forward(kind, U, V, b, uid[keep], pid[keep], nid[keep, None])
        g = mr.grads(kind, U, V, b, uid[keep], pid[keep], nid[keep, None])
        scale = B / keep.sum()                                           # (the mean is over the samples that are kept)
        if kind == "logsig":
            assert abs(loss - want_loss) <= 1e-14 * want_loss and abs(l2 - want_l2) <= 1e-14 * want_l2
        else:
            wl, _, _ = orc.bpr_forward(U, V, b, uid[keep], pid[keep], nid[keep])
            assert abs(loss - wl) <= 1e-13 * wl
        U1 = U[uid[keep]]; P1 = V[pid[keep]]; N1 = V[nid[keep]]
        # the oracle's rows carry l2 with coefficient 1 and its g carries 1/B of the full batch
        assert np.abs(g["gu"] - ((want["gu"][keep] - U1) * scale + U1)).max() <= 1e-13
        assert np.abs(g["gp"] - ((want["gp"][keep] - P1) * scale + P1)).max() <= 1e-13
        assert np.abs(g["gn"][:, 0] - ((want["gn"][keep] - N1) * scale + N1)).max() <= 1e-13
        assert np.abs(g["gbp"] - want["gbp"][keep] * scale).max() <= 1e-14 and np.abs(g["gbn"][:, 0] - want["gbn"][keep] * scale).max() <= 1e-14


def test_an_offset_of_minus_infinity_removes_the_negative_from_the_softmax():
    U, V, b, uid, pid, nid, w, off = _small(6)
    off[:] = np.random.default_rng(7).normal(0, 1, off.shape)
    off[:, 2] = -np.inf
    keep = [0, 1, 3]
    loss, l2 = mr.forward("softmax", U, V, b, uid, pid, nid, w, off)
    g = mr.grads("softmax", U, V, b, uid, pid, nid, w, off, l2_reg=0.0)
    loss1, _ = mr.forward("softmax", U, V, b, uid, pid, nid[:, keep], w, off[:, keep])
    g1 = mr.grads("softmax", U, V, b, uid, pid, nid[:, keep], w, off[:, keep], l2_reg=0.0)
    assert abs(loss - loss1) <= 1e-15
    assert np.array_equal(g["gn"][:, 2], np.zeros_like(g["gn"][:, 2])) and np.array_equal(g["gbn"][:, 2], np.zeros(len(uid)))
    for k in ("gu", "gp", "gbp"):
        assert np.abs(g[k] - g1[k]).max() <= 1e-15, k
    assert np.abs(g["gn"][:, keep] - g1["gn"]).max() <= 1e-15 and np.abs(g["gbn"][:, keep] - g1["gbn"]).max() <= 1e-15


def test_large_logits_stay_finite_in_the_reference():
    U, V, b, uid, pid, nid, w, off = _small(8)
    U *= 30.0; V *= 30.0
    for kind in mr.KINDS:
        loss, _ = mr.forward(kind, U.astype(np.float32), V.astype(np.float32), b.astype(np.float32), uid, pid, nid)
        g = mr.grads(kind, U.astype(np.float32), V.astype(np.float32), b.astype(np.float32), uid, pid, nid)
        assert np.isfinite(loss) and all(np.isfinite(v).all() for v in g.values())


def _run(case, dtype, shuffle_seed=None):
    U, V, b, uid, pid, nid = mc.make(case)
    U, V = U.astype(dtype), V.astype(dtype)
    b = b.astype(dtype) if b is not None else None
    opt = mc.make_opt(case["opt"])
    rng = np.random.default_rng(shuffle_seed) if shuffle_seed is not None else None
    losses = []
    for s in range(case["K"]):
        order = rng.permutation(case["B"] * (1 + case["N"])) if rng is not None else None
        losses.append(mr.step(case["kind"], U, V, b, uid[s], pid[s], nid[s], opt, order=order))
    return U, V, b, losses


@pytest.mark.parametrize("case", mc.CASES, ids=[c["name"] for c in mc.CASES])
def test_headroom_of_the_bounds_on_every_case(case):
    """The float32 reference, with the item occurrences handed over in a shuffled order, passes the GPU test's own check
    against the float64 reference: the bounds leave room for a correct fp32 implementation that sums in another order."""
    from conftest import TOL, TOL_ADAM, rel_err
    U0, V0, b0, _, _, _ = mc.make(case)
    U64, V64, b64, l64 = _run(case, np.float64)
    U32, V32, b32, l32 = _run(case, np.float32, shuffle_seed=case["seed"] + 1)
    tabs = [("user", U0, U32, U64), ("item", V0, V32, V64)] + ([("bias", b0, b32, b64)] if b0 is not None else [])
    for name, W0, got, want in tabs:
        if case["opt"] == "adam":
            assert rel_err(got, want.astype(np.float32)) <= TOL_ADAM, name
        else:
            delta_check(W0, got, want.astype(np.float32), steps=case["K"], what=f"{case['name']} {name}")
    for (a, a2), (w, w2) in zip(l32, l64):
        assert abs(a - w) <= TOL * abs(w) and abs(a2 - w2) <= TOL * abs(w2)


def test_every_optimizer_has_a_duplicate_heavy_case():
    """some item row referenced at least 3 times in one step, as a positive and as a negative, and some user at least twice"""
    for opt in mc.OPTS:
        found = False
        for case in (c for c in mc.CASES if c["opt"] == opt):
            _, _, _, uid, pid, nid = mc.make(case)
            for s in range(case["K"]):
                pos = np.bincount(pid[s], minlength=case["NI"]); neg = np.bincount(nid[s].reshape(-1), minlength=case["NI"])
                both = (pos >= 1) & (neg >= 1) & (pos + neg >= 3)
                found |= bool(both.any()) and np.bincount(uid[s]).max() >= 2
        assert found, opt


def test_the_case_list_covers_the_sizes():
    assert {c["B"] for c in mc.CASES} == {1, 7, 65, 300} and {c["N"] for c in mc.CASES} == {1, 2, 5, 16, 64}
    assert {c["D"] for c in mc.CASES} >= {4, 24, 64, 128, 50, 260}
    for opt in mc.OPTS:
        for kind in mr.KINDS:
            for bias in (True, False):
                assert {c["K"] for c in mc.CASES if (c["opt"], c["kind"], c["bias"]) == (opt, kind, bias)} == {1, 3}


def test_the_three_entry_points_are_declared_typed_and_exposed():
    hdr = open(os.path.join(ROOT, "include", "openrec_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    from openrec_amd import _ffi, runtime as rt
    for name, nargs in (("orx_multineg_step", 19), ("orx_multineg_loss", 15), ("orx_sampler_pairwise_multi", 8)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert m, f"{name} is not declared in openrec_hip.h"
        assert len(m.group(1).split(",")) == nargs, name
        assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == nargs, name
    assert re.search(r"enum\s+orx_multineg_kind\s*\{\s*ORX_MN_SOFTMAX\s*=\s*0\s*,\s*ORX_MN_LOGSIG\s*=\s*1\s*\}", code)
    assert (_ffi.ORX_MN_SOFTMAX, _ffi.ORX_MN_LOGSIG) == (0, 1)
    assert callable(rt.multineg_step) and callable(rt.multineg_loss) and callable(rt.DeviceSampler.pairwise_multi)


def test_bad_arguments_are_value_errors_before_the_library_is_called():
    """(no table handle is ever dereferenced: the stand-ins have only a shape)"""
    from openrec_amd import runtime as rt

    class T:
        def __init__(self, r, d):
            self.shape = (r, d)
    U, V, b = T(10, 8), T(12, 8), T(12, 1)
    uid = np.zeros(4, np.int32); nid = np.zeros((4, 3), np.int32)
    ok = dict(loss="softmax", opt=None, user=U, item=V, bias=b, uid=uid, pid=uid, nid=nid)
    bad = [dict(loss="hinge"), dict(nid=np.zeros(4, np.int32)), dict(nid=np.zeros((4, 65), np.int32)), dict(nid=np.zeros((4, 0), np.int32)),
           dict(user=T(10, 4)), dict(bias=T(11, 1)), dict(bias=T(12, 2)), dict(nid=np.zeros((5, 3), np.int32)), dict(pid=np.zeros(3, np.int32)),
           dict(weights=np.ones(3, np.float32)), dict(neg_offset=np.zeros((4, 2), np.float32)), dict(l2_reg=-1.0), dict(l2_reg=float("nan")),
           dict(l2_reg=0.5, no_l2=True), dict(K=2, B=4), dict(B=4, id_stride=2)]
    for kw in bad:
        with pytest.raises(ValueError):
            rt.multineg_step(**{**ok, **kw})
