"""NumPy restatement of the in-batch softmax (include/openrec_hip.h, orx_inbatch_step), shared by tests/test_inbatch_cpu.py and
tests/test_gpu_inbatch.py.  Everything runs at the dtype of the tables it is given.

    u_i = U[uid[i]],  v_j = V[pid[j]],  b_j = b[pid[j]];   s_ij = scale (u_i . v_j + b_j) + off_j
    hit(i, j) = mask_hits and j != i and pid[j] == pid[i];   N(i) = { j : not hit(i, j) }
    lse_i = logsumexp over N(i) of s_ij;   l_i = lse_i - s_ii
    loss = (1/B) sum_i w_i l_i;   l2_loss = 1/2 (sum |u_i|^2 + sum |v_i|^2);   J = loss + l2_reg * l2_loss
Gradients per occurrence, c_i = w_i / B:
    pi_ij = exp(s_ij - lse_i) on N(i), else 0;   a_ij = c_i pi_ij (j != i),  a_ii = -c_i sum_{j != i} pi_ij
    g_u[i] = scale sum_j a_ij v_j + l2_reg u_i;   g_v[j] = scale sum_i a_ij u_i + l2_reg v_j;   g_b[j] = scale sum_i a_ij
The step hands them to the oracle's optimizers (oracle/numpy_oracle.py, tests/keras_momentum.py), unedited: the user table with
uid, then the item table and the bias with pid."""
import numpy as np

U32 = 2.0 ** -24                                # the unit roundoff of float32


def scores(U, V, b, uid, pid, off=None, scale=1.0):
    """-> u [B, D], v [B, D], s [B, B]"""
    dt = U.dtype
    uid, pid = np.asarray(uid), np.asarray(pid)
    u, v = U[uid], V[pid]
    s = u @ v.T
    if b is not None:
        s = s + b[pid, 0][None, :]
    s = dt.type(scale) * s
    if off is not None:
        s = s + np.asarray(off, dt)[None, :]
    return u, v, s


def columns(pid, mask_hits):
    """-> N [B, B] bool: column j belongs to row i"""
    pid = np.asarray(pid)
    n = np.ones((len(pid), len(pid)), bool)
    if mask_hits:
        n &= ~((pid[None, :] == pid[:, None]) & ~np.eye(len(pid), dtype=bool))
    return n


def _lse(s, n):
    sm = np.where(n, s, -np.inf)
    m = sm.max(1)
    return m + np.log(np.exp(sm - m[:, None]).sum(1))


def row_losses(U, V, b, uid, pid, off=None, scale=1.0, mask_hits=True):
    """-> l [B]"""
    _, _, s = scores(U, V, b, uid, pid, off, scale)
    return _lse(s, columns(pid, mask_hits)) - np.diagonal(s)


def forward(U, V, b, uid, pid, w=None, off=None, scale=1.0, mask_hits=True):
    """-> (loss, l2_loss)"""
    dt = U.dtype
    u, v, s = scores(U, V, b, uid, pid, off, scale)
    l = _lse(s, columns(pid, mask_hits)) - np.diagonal(s)
    wv = np.ones_like(l) if w is None else np.asarray(w, dt)
    loss = (wv * l).sum() / dt.type(len(l))
    return loss, dt.type(0.5) * ((u * u).sum() + (v * v).sum())


def grads(U, V, b, uid, pid, w=None, off=None, scale=1.0, mask_hits=True, l2_reg=1.0):
    """-> dict(gu [B, D], gv [B, D], gb [B])"""
    dt = U.dtype
    u, v, s = scores(U, V, b, uid, pid, off, scale)
    B = len(u)
    n = columns(pid, mask_hits)
    lse = _lse(s, n)
    pi = np.where(n, np.exp(np.where(n, s, -np.inf) - lse[:, None]), 0.0).astype(dt)
    c = (np.ones(B, dt) if w is None else np.asarray(w, dt)) / dt.type(B)
    eye = np.eye(B, dtype=bool)
    A = np.where(eye, 0.0, pi).sum(1)                                  # the off-diagonal pi themselves, never 1 - pi_ii
    a = np.where(eye, -(c * A)[:, None], c[:, None] * pi).astype(dt)
    sc, l2 = dt.type(scale), dt.type(l2_reg)
    return dict(gu=sc * (a @ v) + l2 * u, gv=sc * (a.T @ u) + l2 * v, gb=sc * a.sum(0))


def step(U, V, b, uid, pid, opt, w=None, off=None, scale=1.0, mask_hits=True, l2_reg=1.0, keys=("U", "V", "b")):
    """One train step in place on (U, V, b); b may be None.  Returns (loss, l2_loss) of the pre-step tables."""
    loss, l2 = forward(U, V, b, uid, pid, w, off, scale, mask_hits)
    g = grads(U, V, b, uid, pid, w, off, scale, mask_hits, l2_reg)
    if hasattr(opt, "begin_step"):
        opt.begin_step()
    opt.apply(U, np.asarray(uid), g["gu"], key=keys[0])
    opt.apply(V, np.asarray(pid), g["gv"], key=keys[1])
    if b is not None:
        opt.apply(b, np.asarray(pid), g["gb"][:, None], key=keys[2])
    return loss, l2


def row_bound(U, V, b, uid, pid, off=None, scale=1.0, mask_hits=True):
    """The bound on |l_i (fp32, any summation order) - l_i (exact)| per row, u = 2^-24:
        e_ij    = gamma T_ij,  gamma = (D + 4) u / (1 - (D + 4) u),  T_ij = scale (sum_k |u_ik v_jk| + |b_j|) + |off_j|
        bound_i = max over N(i) of e_ij  +  e_ii  +  (2 B + 32) u  +  2 u (|lse_i| + |s_ii|)
    in order: log-sum-exp is 1-Lipschitz in the maximum norm of the scores' errors; the diagonal; any-order summation of B
    positive terms plus per-tile rescaling and the roundings of the exp arguments (sum_j pi_j t_j <= log B); the roundings of the
    final log and of the subtraction.  Evaluated in float64 from float32 tables."""
    U, V = U.astype(np.float64), V.astype(np.float64)
    b = None if b is None else b.astype(np.float64)
    uid, pid = np.asarray(uid), np.asarray(pid)
    D, B = U.shape[1], len(uid)
    T = np.abs(U[uid]) @ np.abs(V[pid]).T
    if b is not None:
        T = T + np.abs(b[pid, 0])[None, :]
    T = scale * T
    if off is not None:
        T = T + np.abs(np.asarray(off, np.float64))[None, :]
    gamma = (D + 4) * U32 / (1.0 - (D + 4) * U32)
    e = gamma * T
    n = columns(pid, mask_hits)
    _, _, s = scores(U, V, b, uid, pid, None if off is None else np.asarray(off, np.float64), scale)
    lse = _lse(s, n)
    return np.where(n, e, 0.0).max(1) + np.diagonal(e) + (2 * B + 32) * U32 + 2 * U32 * (np.abs(lse) + np.abs(np.diagonal(s)))
