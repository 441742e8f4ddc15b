"""NumPy restatement of the one-positive-against-N-negatives objective (include/openrec_hip.h, orx_multineg_step), shared by
tests/test_multineg_cpu.py and tests/test_gpu_multineg.py.  Everything runs at the dtype of the tables it is given.

Sample i: u = U[uid[i]], p = V[pid[i]], n_j = V[nid[i, j]];  s_p = u.p + b[pid[i]],  s_j = u.n_j + b[nid[i, j]] + off[i, j]
    softmax: l_i = logsumexp(s_p, s_0 .. s_{N-1}) - s_p,                          pi_j = exp(s_j - lse)
    logsig : l_i = (1/N) sum_j -log_sigmoid(max(s_p - s_j, -30))
    loss = (1/B) sum_i w_i l_i;   l2_loss = 1/2 (sum |u|^2 + sum |p|^2 + sum |n|^2);   J = loss + l2_reg * l2_loss
Gradients per occurrence, c_i = w_i / B:
    a_ij = c_i pi_j  |  c_i sigmoid(s_j - s_p) [s_p - s_j >= -30] / N;   A_i = sum_j a_ij
    g_u = sum_j a_ij n_j - A_i p + l2_reg u;  g_p = -A_i u + l2_reg p;  g_nj = a_ij u + l2_reg n_j;  g_bp = -A_i;  g_bnj = a_ij
The step hands them to the oracle's optimizers (oracle/numpy_oracle.py, tests/keras_momentum.py), unedited: the user table with
uid, the item table and the bias with ONE list, pid followed by nid."""
import numpy as np

from oracle import numpy_oracle as orc

KINDS = ("softmax", "logsig")


def _gather(U, V, b, uid, pid, nid, off):
    dt = U.dtype
    uid, pid, nid = np.asarray(uid), np.asarray(pid), np.asarray(nid)
    u, p, n = U[uid], V[pid], V[nid]                                   # [B, D], [B, D], [B, N, D]
    sp = (u * p).sum(1)
    s = (u[:, None, :] * n).sum(2)
    if b is not None:
        sp = sp + b[pid, 0]
        s = s + b[nid, 0]
    if off is not None:
        s = s + np.asarray(off, dt)
    return u, p, n, sp, s


def sample_losses(kind, sp, s):
    """l_i [B] from the scores"""
    if kind == "softmax":
        m = np.maximum(sp, s.max(1))
        tot = np.exp(sp - m) + np.exp(s - m[:, None]).sum(1)
        return m + np.log(tot) - sp
    x = np.maximum(sp[:, None] - s, np.asarray(-30.0, sp.dtype))
    return (-orc.log_sigmoid(x)).mean(1)


def forward(kind, U, V, b, uid, pid, nid, w=None, off=None):
    """-> (loss, l2_loss)"""
    assert kind in KINDS
    u, p, n, sp, s = _gather(U, V, b, uid, pid, nid, off)
    dt = U.dtype
    l = sample_losses(kind, sp, s)
    wv = np.ones_like(l) if w is None else np.asarray(w, dt)
    loss = (wv * l).sum() / dt.type(len(l))
    return loss, orc._l2(u, p, n)


def grads(kind, U, V, b, uid, pid, nid, w=None, off=None, l2_reg=1.0):
    """-> dict(gu [B, D], gp [B, D], gn [B, N, D], gbp [B], gbn [B, N])"""
    assert kind in KINDS
    u, p, n, sp, s = _gather(U, V, b, uid, pid, nid, off)
    dt = U.dtype
    B, N = s.shape
    c = (np.ones(B, dt) if w is None else np.asarray(w, dt)) / dt.type(B)
    if kind == "softmax":
        m = np.maximum(sp, s.max(1))
        e = np.exp(s - m[:, None])
        tot = np.exp(sp - m) + e.sum(1)
        a = c[:, None] * e / tot[:, None]
    else:
        x = sp[:, None] - s
        with np.errstate(invalid="ignore"):
            a = c[:, None] * orc._sigmoid(-x) * (x >= -30.0) / dt.type(N)
    a = a.astype(dt)
    A = a.sum(1)                                                       # the pi_j themselves, never 1 - pi_p
    l2 = dt.type(l2_reg)
    gu = (a[:, :, None] * n).sum(1) - A[:, None] * p + l2 * u
    gp = -A[:, None] * u + l2 * p
    gn = a[:, :, None] * u[:, None, :] + l2 * n
    return dict(gu=gu, gp=gp, gn=gn, gbp=-A, gbn=a)


def step(kind, U, V, b, uid, pid, nid, opt, w=None, off=None, l2_reg=1.0, keys=("U", "V", "b"), order=None):
    """One train step in place on (U, V, b); b may be None.  Returns (loss, l2_loss) of the pre-step tables.
    order: a permutation of the (1 + N) B item occurrences -- the list and its gradient rows are handed over in that order (the
    result may then differ by summation order only)."""
    loss, l2 = forward(kind, U, V, b, uid, pid, nid, w, off)
    g = grads(kind, U, V, b, uid, pid, nid, w, off, l2_reg)
    D = U.shape[1]
    ids = np.concatenate([np.asarray(pid).reshape(-1), np.asarray(nid).reshape(-1)])
    G = np.concatenate([g["gp"], g["gn"].reshape(-1, D)])
    Gb = np.concatenate([g["gbp"], g["gbn"].reshape(-1)])[:, None]
    if order is not None:
        ids, G, Gb = ids[order], G[order], Gb[order]
    if hasattr(opt, "begin_step"):
        opt.begin_step()
    opt.apply(U, np.asarray(uid), g["gu"], key=keys[0])
    opt.apply(V, ids, G, key=keys[1])
    if b is not None:
        opt.apply(b, ids, Gb, key=keys[2])
    return loss, l2
