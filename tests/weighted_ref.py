"""The expected result of a train step with per-triplet weights and an l2 coefficient, composed from the unchanged oracle
(oracle/numpy_oracle.py).

Objective of one step (include/openrec_hip.h, orx_pairwise_step_weighted):

    BPR : loss = (1/B) sum_i w_i * (-log_sigmoid(max(x_i, -30)))        UCML: loss = sum_i w_i * max(margin - diff_i, 0)
    J    = loss + l2_reg * l2_loss                                      (l2_loss: the model's own term, never weighted)

The oracle's `*_grads` return the per-occurrence gradients of loss + 1 * l2_loss and the coefficient `g` of the loss part
(BPR: d loss / d x_i; UCML: the hinge indicator; GMF / WRMF: d loss / d score).  Mathematically the weighted gradient of a
row is w * (g_full - row) + l2_reg * row.  It is FORMED here from the oracle's coefficient in the oracle's own expression,
(w * g) * A + l2_reg * row, because floating point does not give (c*A + row) - row == c*A: only this form equals the oracle's
step bit for bit at w = 1, l2_reg = 1 (tests/test_weighted_cpu.py holds both facts: the exact equality, and the agreement of
the two forms to 1e-12 in float64).  Gradients are taken on the pre-step tables; the optimizers are the oracle's and
tests/subset_expect.Momentum; only the trained roles are applied.  Shared by tests/test_weighted_cpu.py (against fixtures minted
from the reference's own class text, tests/golden/make_golden_l2reg.py) and tests/test_gpu_weighted.py."""
import numpy as np

from oracle import numpy_oracle as orc

ALL = ("user", "item", "bias")


def pair_forward(model, U, V, b, uid, pid, nid, w=None, margin=0.5):
    """(weighted loss, unscaled l2_loss)"""
    if model == "bpr":
        _, l2, x = orc.bpr_forward(U, V, b, uid, pid, nid)
        per = -orc.log_sigmoid(np.maximum(x, np.asarray(-30.0, x.dtype)))
        per = per if w is None else per * np.asarray(w, x.dtype)
        return per.mean(dtype=x.dtype), l2
    _, l2, h = orc.ucml_forward(U, V, b, uid, pid, nid, margin)
    per = np.maximum(h, 0)
    per = per if w is None else per * np.asarray(w, h.dtype)
    return per.sum(dtype=h.dtype), l2


def pair_grads(model, U, V, b, uid, pid, nid, w=None, l2_reg=1.0, margin=0.5):
    """per-occurrence gradients of J on the gathered rows: dict(gu, gp, gn [B, D]; gbp, gbn [B])"""
    u, p, n = U[uid], V[pid], V[nid]
    dt = u.dtype.type
    gr = orc.bpr_grads(U, V, b, uid, pid, nid) if model == "bpr" else orc.ucml_grads(U, V, b, uid, pid, nid, margin)
    g = gr["g"] if w is None else np.asarray(w, u.dtype) * gr["g"]
    lam = dt(l2_reg)
    if model == "bpr":
        return dict(gu=g[:, None] * (p - n) + lam * u, gp=g[:, None] * u + lam * p, gn=-g[:, None] * u + lam * n, gbp=g, gbn=-g)
    return dict(gu=-2 * g[:, None] * (p - n) + lam * u, gp=-2 * g[:, None] * (u - p) + lam * p, gn=2 * g[:, None] * (u - n) + lam * n,
                gbp=-g, gbn=g)


def pair_grads_by_difference(model, U, V, b, uid, pid, nid, w, l2_reg, margin=0.5):
    """the same gradients as the issue states them: w * (g_full - row) + l2_reg * row, w * gbp, w * gbn"""
    u, p, n = U[uid], V[pid], V[nid]
    gr = orc.bpr_grads(U, V, b, uid, pid, nid) if model == "bpr" else orc.ucml_grads(U, V, b, uid, pid, nid, margin)
    w = np.asarray(w, u.dtype)
    lam = u.dtype.type(l2_reg)
    return dict(gu=w[:, None] * (gr["gu"] - u) + lam * u, gp=w[:, None] * (gr["gp"] - p) + lam * p, gn=w[:, None] * (gr["gn"] - n) + lam * n,
                gbp=w * gr["gbp"], gbn=w * gr["gbn"])


def pair_step(model, U, V, b, uid, pid, nid, oo, w=None, l2_reg=1.0, roles=ALL, margin=0.5, censor=False):
    """one weighted step on the trained roles; U, V, b (b may be None: bias-free BPR) are updated in place; returns (loss, l2)"""
    bb = b if b is not None else np.zeros((V.shape[0], 1), V.dtype)
    loss, l2 = pair_forward(model, U, V, bb, uid, pid, nid, w, margin)
    gr = pair_grads(model, U, V, bb, uid, pid, nid, w, l2_reg, margin)
    item_ids = np.concatenate([pid, nid])
    if hasattr(oo, "begin_step"):
        oo.begin_step()
    if "user" in roles:
        oo.apply(U, uid, gr["gu"], key="U")
    if "item" in roles:
        oo.apply(V, item_ids, np.concatenate([gr["gp"], gr["gn"]]), key="V")
    if "bias" in roles and b is not None:
        oo.apply(b, item_ids, np.concatenate([gr["gbp"], gr["gbn"]])[:, None], key="b")
    if censor:                                  # ucml.py:44-48
        orc.censor(U, uid); orc.censor(V, pid); orc.censor(V, nid)
    return loss, l2


def point_step(model, U, V, b, wd, uid, iid, label, oo, l2_reg=1.0, roles=ALL, a=1.0, b_w=1.0, sigmoid=False):
    """one GMF (wd: the Dense kernel [D, 1]) / WRMF (wd None) step of J = loss + l2_reg * l2_loss; returns (loss, unscaled l2)"""
    u, i = U[uid], V[iid]
    lam = u.dtype.type(l2_reg)
    if model == "gmf":
        loss, l2, _ = orc.gmf_forward(U, V, b, wd, uid, iid, label)
        gs = orc.gmf_grads(U, V, b, wd, uid, iid, label)["g"]
        gu = gs[:, None] * (i * wd[:, 0][None, :]) + lam * u
        gi = gs[:, None] * (u * wd[:, 0][None, :]) + lam * i
        gw = ((u * i) * gs[:, None]).sum(0, dtype=u.dtype)[:, None] + lam * wd
    else:
        loss, l2, _ = orc.wrmf_forward(U, V, b, uid, iid, label, a, b_w, sigmoid)
        gs = orc.wrmf_grads(U, V, b, uid, iid, label, a, b_w, sigmoid)["g"]
        gu = gs[:, None] * i + lam * u
        gi = gs[:, None] * u + lam * i
    if hasattr(oo, "begin_step"):
        oo.begin_step()
    if "user" in roles:
        oo.apply(U, uid, gu, key="U")
    if "item" in roles:
        oo.apply(V, iid, gi, key="V")
    if "bias" in roles:
        oo.apply(b, iid, gs[:, None], key="b")
    if model == "gmf":
        oo.apply_dense(wd, gw, key="w")
    return loss, l2
