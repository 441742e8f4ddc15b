"""NumPy restatement of the history-pooled sequence recommender (include/openrec_hip.h, orx_bag_pool / orx_seqrec_step), shared by
tests/test_seqrec_cpu.py and tests/test_gpu_seqrec.py.  Everything runs at the dtype of the tables it is given.

    q_i = c_i * sum over e in bag i, in list order, of H[items[e]]      c_i = 1 / len_i ("mean") | 1 ("sum") | 1 / denom (("fixed", denom))
The objective is tests/multineg_ref.py's on (Q, V, b) with uid = arange(B): the l2 term sits on the pooled vector.  Occurrence e of
bag i has the gradient row c_i * g_q[i]; the step hands the n occurrence rows with the list `items` to the oracle's optimizers
(oracle/numpy_oracle.py, tests/keras_momentum.py), then the item table and the bias with ONE list, pid followed by nid, as
multineg_ref.step does."""
import numpy as np

import multineg_ref as mr

KINDS = mr.KINDS
U24 = 2.0 ** -24


def coefs(ptr, pool, dt):
    """c_i [B] at dtype dt: rounded once when dt is float32; 0 for an empty bag"""
    lens = np.diff(np.asarray(ptr, np.int64))
    one = dt.type(1)
    if pool == "mean":
        with np.errstate(divide="ignore"):
            c = np.where(lens > 0, one / np.maximum(lens, 1).astype(dt), dt.type(0))
        return c.astype(dt)
    denom = 1.0 if pool == "sum" else pool[1]
    assert pool == "sum" or pool[0] == "fixed"
    return np.where(lens > 0, one / dt.type(denom), dt.type(0)).astype(dt)


def pool_rows(H, ptr, items, pool):
    """-> Q [B, D], c [B]: the rows added in list order at H's dtype, the product rounded once; an empty bag gives +0"""
    dt = H.dtype
    ptr = np.asarray(ptr, np.int64)
    B = len(ptr) - 1
    c = coefs(ptr, pool, dt)
    Q = np.zeros((B, H.shape[1]), dt)
    for i in range(B):
        lo, hi = ptr[i], ptr[i + 1]
        if hi > lo:
            Q[i] = c[i] * np.add.accumulate(H[np.asarray(items[lo:hi])], axis=0, dtype=dt)[-1]
    return Q, c


def pool_bound(H, ptr, items, c):
    """[B, D]: (len_i + 1) 2^-24 / (1 - (len_i + 1) 2^-24) * |c_i| * sum_e |H[item_e]| -- the standard bound of an fp32 sum of len_i
    terms in ANY order (len_i - 1 roundings on a path), c_i rounded once, one product"""
    ptr = np.asarray(ptr, np.int64)
    B = len(ptr) - 1
    A = np.abs(np.asarray(H, np.float64))
    out = np.zeros((B, H.shape[1]))
    for i in range(B):
        lo, hi = ptr[i], ptr[i + 1]
        k = (hi - lo + 1) * U24
        out[i] = k / (1.0 - k) * abs(float(c[i])) * A[np.asarray(items[lo:hi])].sum(0)
    return out


def owners(ptr):
    """[n]: the bag of every list position"""
    ptr = np.asarray(ptr, np.int64)
    return np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))


def forward(kind, H, V, b, ptr, items, pid, nid, pool, w=None, off=None):
    """-> (loss, l2_loss)"""
    Q, _ = pool_rows(H, ptr, items, pool)
    return mr.forward(kind, Q, V, b, np.arange(len(Q)), pid, nid, w, off)


def grads(kind, H, V, b, ptr, items, pid, nid, pool, w=None, off=None, l2_reg=0.0):
    """-> multineg_ref.grads' dict on (Q, V, b) plus gh [n, D], the occurrence rows of the history table"""
    Q, c = pool_rows(H, ptr, items, pool)
    g = mr.grads(kind, Q, V, b, np.arange(len(Q)), pid, nid, w, off, l2_reg)
    own = owners(ptr)
    g["gh"] = (c[own, None] * g["gu"][own]).astype(H.dtype)
    return g


def step(kind, H, V, b, ptr, items, pid, nid, opt, pool, w=None, off=None, l2_reg=0.0, keys=("H", "V", "b")):
    """One train step in place on (H, V, b); b may be None.  Returns (loss, l2_loss) of the pre-step tables."""
    loss, l2 = forward(kind, H, V, b, ptr, items, pid, nid, pool, w, off)
    g = grads(kind, H, V, b, ptr, items, pid, nid, pool, w, off, l2_reg)
    D = H.shape[1]
    ids = np.concatenate([np.asarray(pid).reshape(-1), np.asarray(nid).reshape(-1)])
    G = np.concatenate([g["gp"], g["gn"].reshape(-1, D)])
    Gb = np.concatenate([g["gbp"], g["gbn"].reshape(-1)])[:, None]
    if hasattr(opt, "begin_step"):
        opt.begin_step()
    if len(items):
        opt.apply(H, np.asarray(items), g["gh"], key=keys[0])
    opt.apply(V, ids, G, key=keys[1])
    if b is not None:
        opt.apply(b, ids, Gb, key=keys[2])
    return loss, l2
