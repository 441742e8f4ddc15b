"""NumPy restatement of the full softmax over all items (include/openrec_hip.h, orx_fullsoftmax_step / orx_seqrec_full_step),
shared by tests/test_fullsoftmax_cpu.py and tests/test_gpu_fullsoftmax.py.  Everything runs at the dtype of the tables it is given.

    u_i = U[uid[i]];   s_ij = scale (u_i . V[j] + b[j]) + off[j],  j over ALL NI items
    lse_i = logsumexp_j s_ij;   l_i = lse_i - s_{i,pid[i]}
    loss = (1/B) sum_i w_i l_i;   l2_loss = 1/2 (sum |u_i|^2 + sum |V[pid[i]]|^2);   J = loss + l2_reg * l2_loss
Gradients, c_i = w_i / B, n_j = the number of samples whose label is j:
    pi_ij = exp(s_ij - lse_i);   a_ij = c_i pi_ij (j != pid[i]),  a_{i,pid[i]} = -c_i sum_{j != pid[i]} pi_ij
    gu[i] = scale sum_j a_ij V[j] + l2_reg u_i;   GV[j] = scale sum_i a_ij u_i + l2_reg n_j V[j];   Gb[j] = scale sum_i a_ij
The step hands gu to the sparse `apply` of the oracle's optimizers (oracle/numpy_oracle.py, tests/keras_momentum.py, unedited)
with uid, and GV / Gb to their `apply_dense`.  The SeqRec form pools the query rows with tests/seqrec_ref.py and hands the
occurrence rows c_i * g_q[i] of the history table to `apply` with the list of the bags."""
import numpy as np

import seqrec_ref as sr

U32 = 2.0 ** -24                                # the unit roundoff of float32


def scores(Q, V, b, off=None, scale=1.0):
    """Q [B, D] query rows -> s [B, NI]"""
    dt = Q.dtype
    s = Q @ V.T
    if b is not None:
        s = s + b[:, 0][None, :]
    s = dt.type(scale) * s
    if off is not None:
        s = s + np.asarray(off, dt)[None, :]
    return s


def _lse(s):
    m = s.max(1)
    return m + np.log(np.exp(s - m[:, None]).sum(1))


def _label(s, pid):
    return s[np.arange(len(pid)), np.asarray(pid)]


def row_losses_q(Q, V, b, pid, off=None, scale=1.0):
    s = scores(Q, V, b, off, scale)
    return _lse(s) - _label(s, pid)


def row_losses(U, V, b, uid, pid, off=None, scale=1.0):
    """-> l [B]"""
    return row_losses_q(U[np.asarray(uid)], V, b, pid, off, scale)


def forward_q(Q, V, b, pid, w=None, off=None, scale=1.0):
    dt = Q.dtype
    l = row_losses_q(Q, V, b, pid, off, scale)
    wv = np.ones_like(l) if w is None else np.asarray(w, dt)
    v = V[np.asarray(pid)]
    return (wv * l).sum() / dt.type(len(l)), dt.type(0.5) * ((Q * Q).sum() + (v * v).sum())


def forward(U, V, b, uid, pid, w=None, off=None, scale=1.0):
    """-> (loss, l2_loss)"""
    return forward_q(U[np.asarray(uid)], V, b, pid, w, off, scale)


def coefficients(Q, V, b, pid, w=None, off=None, scale=1.0):
    """-> a [B, NI], pi [B, NI]"""
    dt = Q.dtype
    pid = np.asarray(pid)
    B = len(pid)
    s = scores(Q, V, b, off, scale)
    pi = np.exp(s - _lse(s)[:, None]).astype(dt)
    c = (np.ones(B, dt) if w is None else np.asarray(w, dt)) / dt.type(B)
    lab = np.zeros(s.shape, bool)
    lab[np.arange(B), pid] = True
    A = np.where(lab, 0.0, pi).sum(1)                                  # the other items' pi themselves, never 1 - pi_label
    return np.where(lab, -(c * A)[:, None], c[:, None] * pi).astype(dt), pi


def grads_q(Q, V, b, pid, w=None, off=None, scale=1.0, l2_reg=0.0):
    dt = Q.dtype
    a, _ = coefficients(Q, V, b, pid, w, off, scale)
    n = np.bincount(np.asarray(pid), minlength=len(V)).astype(dt)
    sc, l2 = dt.type(scale), dt.type(l2_reg)
    return dict(gu=sc * (a @ V) + l2 * Q, GV=sc * (a.T @ Q) + (l2 * n)[:, None] * V, Gb=sc * a.sum(0))


def grads(U, V, b, uid, pid, w=None, off=None, scale=1.0, l2_reg=0.0):
    """-> dict(gu [B, D], GV [NI, D], Gb [NI])"""
    return grads_q(U[np.asarray(uid)], V, b, pid, w, off, scale, l2_reg)


def _apply_items(opt, V, b, g, train, keys):
    if "item" in train:
        opt.apply_dense(V, g["GV"], key=keys[1])
    if b is not None and "bias" in train:
        opt.apply_dense(b, g["Gb"][:, None], key=keys[2])


def step(U, V, b, uid, pid, opt, w=None, off=None, scale=1.0, l2_reg=0.0, train=("user", "item", "bias"), keys=("U", "V", "b")):
    """One train step in place on (U, V, b); b may be None.  Returns (loss, l2_loss) of the pre-step tables."""
    loss, l2 = forward(U, V, b, uid, pid, w, off, scale)
    g = grads(U, V, b, uid, pid, w, off, scale, l2_reg)
    if hasattr(opt, "begin_step"):
        opt.begin_step()
    if "user" in train:
        opt.apply(U, np.asarray(uid), g["gu"], key=keys[0])
    _apply_items(opt, V, b, g, train, keys)
    return loss, l2


def row_bound_q(Q, V, b, pid, off=None, scale=1.0):
    Q, V = Q.astype(np.float64), V.astype(np.float64)
    b = None if b is None else b.astype(np.float64)
    off = None if off is None else np.asarray(off, np.float64)
    D, NI = V.shape[1], V.shape[0]
    T = np.abs(Q) @ np.abs(V).T
    if b is not None:
        T = T + np.abs(b[:, 0])[None, :]
    T = scale * T
    if off is not None:
        T = T + np.where(np.isfinite(off), np.abs(off), 0.0)[None, :]           # (a removed item has no score to be wrong)
    gamma = (D + 4) * U32 / (1.0 - (D + 4) * U32)
    e = gamma * T
    s = scores(Q, V, b, off, scale)
    lse, sl = _lse(s), _label(s, pid)
    return e.max(1) + _label(e, pid) + (2 * NI + 32) * U32 + 2 * U32 * (np.abs(lse) + np.abs(sl))


def row_bound(U, V, b, uid, pid, off=None, scale=1.0):
    """inbatch_ref.row_bound with the columns being all items: the bound on |l_i (fp32, any summation order) - l_i (exact)|,
        e_ij    = gamma T_ij,  gamma = (D + 4) u / (1 - (D + 4) u),  T_ij = scale (sum_k |u_ik V_jk| + |b_j|) + |off_j|
        bound_i = max_j e_ij + e_{i,label} + (2 NI + 32) u + 2 u (|lse_i| + |s_label|)
    Evaluated in float64 from float32 tables."""
    return row_bound_q(U[np.asarray(uid)], V, b, pid, off, scale)


# ---- the SeqRec form: the query rows are pooled (tests/seqrec_ref.py), the history table takes the occurrence rows -----------------
def seq_forward(H, V, b, ptr, items, pid, pool, w=None, off=None, scale=1.0):
    Q, _ = sr.pool_rows(H, ptr, items, pool)
    return forward_q(Q, V, b, pid, w, off, scale)


def seq_row_losses(H, V, b, ptr, items, pid, pool, off=None, scale=1.0):
    Q, _ = sr.pool_rows(H, ptr, items, pool)
    return row_losses_q(Q, V, b, pid, off, scale)


def seq_step(H, V, b, ptr, items, pid, opt, pool, w=None, off=None, scale=1.0, l2_reg=0.0, train=("history", "item", "bias"),
             keys=("H", "V", "b")):
    """One train step in place on (H, V, b); returns (loss, l2_loss) of the pre-step tables"""
    Q, c = sr.pool_rows(H, ptr, items, pool)
    loss, l2 = forward_q(Q, V, b, pid, w, off, scale)
    g = grads_q(Q, V, b, pid, w, off, scale, l2_reg)
    own = sr.owners(ptr)
    gh = (c[own, None] * g["gu"][own]).astype(H.dtype)
    if hasattr(opt, "begin_step"):
        opt.begin_step()
    if "history" in train and len(items):
        opt.apply(H, np.asarray(items), gh, key=keys[0])
    _apply_items(opt, V, b, g, train, keys)
    return loss, l2
