"""References of the VBPR step (include/openrec_hip.h, "VBPR") for tests/test_vbpr_cpu.py and tests/test_gpu_vbpr.py.

Two independent ones, both run in the dtype of their inputs (float64 for a reference, float32 for the headroom checks):
  grads        the issue's formulas by hand in NumPy -- the pair difference df = F[p] - F[n], Delta = df E, per-occurrence gradient
               rows, dE = df^T R + l2_proj E --, np.add.at where duplicates are summed;
  torch_grads  the score written directly (theta = F @ E for ALL items, gather, softplus) under torch float64 autograd, whose
               embedding backward is a dense index_add.  It knows nothing of the df shortcut.
`step` applies `grads` with the optimizer rules of oracle/numpy_oracle.py (SGD, Adagrad, TF-2.0 Adam) and tests/keras_momentum.py,
the projection by their dense rule.  The two bounds are the worst case of an fp32 fma chain of that length in ANY order
(u = 2^-24 per product and per add, (n + small) u sum |a b| in all):
  proj_bound   (Fd + 8) u (|F[ia] - F[ib]| |E|)            for the projection
  dproj_bound  (chunk_rows + chunks + 8) u (|df|^T |R|)     for dE summed over `chunks` partials of `chunk_rows` triplets each"""
import numpy as np

U32 = 2.0 ** -24


def _logsig_terms(x):
    """-> (-log_sigmoid(max(x, -30)), sigmoid(-x) [x >= -30]) in x's dtype"""
    m = np.maximum(x, x.dtype.type(-30))
    e = np.exp(-np.abs(m))
    term = np.maximum(-m, 0) + np.log1p(e)
    sig = np.where(x >= 0, e / (1 + e), 1 / (1 + e))
    return term, np.where(x >= -30, sig, 0).astype(x.dtype)


def grads(U, V, b, E, F, uid, pid, nid, w=None, l2_reg=0.0, l2_proj=0.0):
    """-> dict: loss, l2 (unscaled), per-occurrence gu [B, D], gp / gn [B, Dl], gbp / gbn [B], dense dE [Fd, Dc], and the
    intermediates df [B, Fd], delta [B, Dc], R [B, Dc], x [B]"""
    dt = U.dtype.type
    Dl = V.shape[1]
    B = len(uid)
    F = F.astype(U.dtype)
    u, p, n = U[uid], V[pid], V[nid]
    ul, uc = u[:, :Dl], u[:, Dl:]
    df = F[pid] - F[nid]
    delta = df @ E
    x = (ul * (p - n)).sum(1) + (uc * delta).sum(1)
    if b is not None:
        x = x + b[pid, 0] - b[nid, 0]
    term, sig = _logsig_terms(x)
    wk = np.ones(B, U.dtype) if w is None else w.astype(U.dtype)
    loss = (wk * term).sum() / dt(B)
    l2 = dt(0.5) * ((u * u).sum() + (p * p).sum() + (n * n).sum())
    g = -wk * sig / dt(B)
    lr = dt(l2_reg)
    gu = np.concatenate([g[:, None] * (p - n), g[:, None] * delta], 1) + lr * u
    gp = g[:, None] * ul + lr * p
    gn = -g[:, None] * ul + lr * n
    R = g[:, None] * uc
    dE = df.T @ R + dt(l2_proj) * E
    return dict(loss=loss, l2=l2, gu=gu, gp=gp, gn=gn, gbp=g, gbn=-g, dE=dE, df=df, delta=delta, R=R, x=x)


def dense(gr, shapes, uid, pid, nid):
    """the per-occurrence rows of `grads` summed into dense (GU, GV, Gb) of the tables' shapes (np.add.at)"""
    (NU, D), (NI, Dl) = shapes
    GU = np.zeros((NU, D), gr["gu"].dtype); GV = np.zeros((NI, Dl), GU.dtype); Gb = np.zeros((NI, 1), GU.dtype)
    np.add.at(GU, uid, gr["gu"])
    np.add.at(GV, pid, gr["gp"]); np.add.at(GV, nid, gr["gn"])
    np.add.at(Gb[:, 0], pid, gr["gbp"]); np.add.at(Gb[:, 0], nid, gr["gbn"])
    return GU, GV, Gb


def torch_grads(U, V, b, E, F, uid, pid, nid, w=None, l2_reg=0.0, l2_proj=0.0):
    """float64 autograd of J = loss + l2_reg l2_loss + l2_proj / 2 |E|^2 with the score written directly
    -> dict: loss, l2, dense GU, GV, Gb (None without b), dE"""
    import torch
    t = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    tU, tV, tE = t(U), t(V), t(E)
    tb = t(b) if b is not None else None
    tF = torch.tensor(np.asarray(F, np.float64))
    iu, ip, inn = (torch.as_tensor(np.asarray(a, np.int64)) for a in (uid, pid, nid))
    Dl = V.shape[1]
    theta = tF @ tE                                           # every item's content vector

    def s(i):
        out = (tU[iu][:, :Dl] * tV[i]).sum(1) + (tU[iu][:, Dl:] * theta[i]).sum(1)
        return out + tb[i, 0] if tb is not None else out

    x = s(ip) - s(inn)
    wk = torch.ones(len(uid), dtype=torch.float64) if w is None else torch.tensor(np.asarray(w, np.float64))
    loss = (wk * torch.nn.functional.softplus(-torch.clamp(x, min=-30.0))).mean()
    l2 = 0.5 * ((tU[iu] ** 2).sum() + (tV[ip] ** 2).sum() + (tV[inn] ** 2).sum())
    J = loss + l2_reg * l2 + l2_proj * 0.5 * (tE ** 2).sum()
    J.backward()
    g = lambda v: v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))
    return dict(loss=float(loss.detach()), l2=float(l2.detach()), GU=g(tU), GV=g(tV), Gb=g(tb) if tb is not None else None, dE=g(tE))


ROLES = ("user", "item", "bias", "proj")


def step(U, V, b, E, F, uid, pid, nid, opt, w=None, l2_reg=0.0, l2_proj=0.0, train=None):
    """one train step in place on (U, V, b, E) with `grads` and the optimizer's rules; train: None or the roles to update
    -> (loss, l2)"""
    gr = grads(U, V, b, E, F, uid, pid, nid, w, l2_reg, l2_proj)
    on = set(ROLES if train is None else train)
    if hasattr(opt, "begin_step"):
        opt.begin_step()
    both = np.concatenate([pid, nid])
    if "user" in on:
        opt.apply(U, uid, gr["gu"], key="U")
    if "item" in on:
        opt.apply(V, both, np.concatenate([gr["gp"], gr["gn"]]), key="V")
    if "bias" in on and b is not None:
        opt.apply(b, both, np.concatenate([gr["gbp"], gr["gbn"]])[:, None], key="b")
    if "proj" in on:
        opt.apply_dense(E, gr["dE"].astype(E.dtype), key="E")
    return float(gr["loss"]), float(gr["l2"])


def make_opt(name, lr=None):
    """the optimizers of the cases (tests/vbpr_cases.py has the learning rates); the device's take the same constants"""
    from oracle import numpy_oracle as orc
    from keras_momentum import Momentum
    import vbpr_cases as vc
    lr = vc.LR[name] if lr is None else lr
    if name == "sgd":
        return orc.SGD(lr)
    if name == "adagrad":
        return orc.Adagrad(lr)
    if name == "adam":
        return orc.AdamTFSparse(lr)
    return Momentum(lr, 0.9, True)


def theta(F, E):
    """float64 F E"""
    return np.asarray(F, np.float64) @ np.asarray(E, np.float64)


def project(F, E, ia, ib=None):
    """float64 (F[ia] - F[ib]) E"""
    F = np.asarray(F, np.float64)
    d = F[ia] - (F[ib] if ib is not None else 0.0)
    return d @ np.asarray(E, np.float64)


def proj_bound(F, E, ia, ib=None):
    F = np.asarray(F, np.float64)
    d = np.abs(F[ia] - (F[ib] if ib is not None else 0.0))
    return (F.shape[1] + 8) * U32 * (d @ np.abs(np.asarray(E, np.float64)))


def dproj_bound(df, R, chunk_rows, chunks):
    return (chunk_rows + chunks + 8) * U32 * (np.abs(np.asarray(df, np.float64)).T @ np.abs(np.asarray(R, np.float64)))
