"""NumPy restatement of the history-pooled recommender with a dense tower (include/openrec_hip.h, orx_tower_step), shared by
tests/test_tower_cpu.py and tests/test_gpu_tower.py.  Everything runs at the dtype of the tables it is given.

    x0_i = [ S_1[f_1[i]] | ... | S_m[f_m[i]] | pool(H[bag_i]) ];   x_{l+1} = act(x_l W_l + c_l);   q_i = x_L
    loss, the row losses and the item side as tests/fullsoftmax_ref.py has them on Q = x_L
    l2_loss = 1/2 (sum |x0_i|^2 + sum |V[pid[i]]|^2);   J = loss + l2_reg l2_loss + l2_mlp 1/2 sum_l (|W_l|^2 + |c_l|^2)
act is relu with relu'(0) = 0; the last layer's only with relu_last.  The pool is tests/seqrec_ref.pool_rows, the query gradient
fullsoftmax_ref.grads_q (with l2_reg = 0 on the query: the term sits on x0).  The step hands the occurrence rows c_i g_0[i][so:]
of the history table and the column slices of g_0 with their id lists to the sparse `apply` of the oracle's optimizers, and
G_V, G_b, dW_l, dc_l to their `apply_dense`.  A model is (H, V, b, S, layers): S a list of tables, layers a list of [W, c]
(c [1, out] or None)."""
import numpy as np

import fullsoftmax_ref as fr
import seqrec_ref as sr

ROLES = ("history", "item", "bias", "side", "tower")


def input_rows(H, S, ptr, items, f, pool):
    """-> x0 [B, in_0], c [B], so (the pool's first column)"""
    P, c = sr.pool_rows(H, ptr, items, pool)
    parts = [Sj[np.asarray(fj)] for Sj, fj in zip(S, f)] + [P]
    return np.concatenate(parts, axis=1).astype(H.dtype), c, sum(Sj.shape[1] for Sj in S)


def tower(x0, layers, relu_last=True):
    """-> xs [x_0 .. x_L], zs the pre-activations [z_1 .. z_L]"""
    xs, zs = [x0], []
    for l, (W, c) in enumerate(layers):
        z = xs[-1] @ W
        if c is not None:
            z = z + c[0][None, :]
        zs.append(z)
        relu = l + 1 < len(layers) or relu_last
        xs.append(np.where(z > 0, z, z.dtype.type(0)) if relu else z)
    return xs, zs


def queries(H, S, layers, ptr, items, f, pool, relu_last=True):
    x0, _, _ = input_rows(H, S, ptr, items, f, pool)
    return tower(x0, layers, relu_last)[0][-1]


def forward(H, V, b, S, layers, ptr, items, f, pid, pool, relu_last=True, w=None, off=None, scale=1.0):
    """-> (loss, l2_loss)"""
    dt = H.dtype
    x0, _, _ = input_rows(H, S, ptr, items, f, pool)
    Q = tower(x0, layers, relu_last)[0][-1]
    loss, _ = fr.forward_q(Q, V, b, pid, w, off, scale)
    v = V[np.asarray(pid)]
    return loss, dt.type(0.5) * ((x0 * x0).sum() + (v * v).sum())


def row_losses(H, V, b, S, layers, ptr, items, f, pid, pool, relu_last=True, off=None, scale=1.0):
    return fr.row_losses_q(queries(H, S, layers, ptr, items, f, pool, relu_last), V, b, pid, off, scale)


def grads(H, V, b, S, layers, ptr, items, f, pid, pool, relu_last=True, w=None, off=None, scale=1.0, l2_reg=0.0, l2_mlp=0.0):
    """-> dict(GV, Gb, dW [L], dc [L] (None where c_l is), g0 [B, in_0], gh [n, Dh], gS [m] of [B, d_j])"""
    dt = H.dtype
    x0, c, so = input_rows(H, S, ptr, items, f, pool)
    xs, _ = tower(x0, layers, relu_last)
    Q = xs[-1]
    gq = fr.grads_q(Q, V, b, pid, w, off, scale, 0.0)["gu"]                 # (no l2 on the query itself)
    gi = fr.grads_q(Q, V, b, pid, w, off, scale, l2_reg)
    l2, lm = dt.type(l2_reg), dt.type(l2_mlp)
    L = len(layers)
    dW, dc = [None] * L, [None] * L
    g = gq
    for l in range(L - 1, -1, -1):
        W, cl = layers[l]
        relu = l + 1 < L or relu_last
        gm = np.where(xs[l + 1] > 0, g, dt.type(0)) if relu else g
        dW[l] = xs[l].T @ gm + lm * W
        if cl is not None:
            dc[l] = gm.sum(0)[None, :] + lm * cl
        g = gm @ W.T
    g0 = (g + l2 * x0).astype(dt)
    own = sr.owners(ptr)
    gh = (c[own, None] * g0[own, so:]).astype(dt)
    gS, c0 = [], 0
    for Sj in S:
        gS.append(np.ascontiguousarray(g0[:, c0:c0 + Sj.shape[1]]))
        c0 += Sj.shape[1]
    return dict(GV=gi["GV"], Gb=gi["Gb"], dW=dW, dc=dc, g0=g0, gh=gh, gS=gS, gq=gq)


def step(H, V, b, S, layers, ptr, items, f, pid, opt, pool, relu_last=True, w=None, off=None, scale=1.0, l2_reg=0.0, l2_mlp=0.0,
         train=ROLES):
    """One train step in place on every table of the model; returns (loss, l2_loss) of the pre-step tables.  The optimizer's keys:
    "H", "V", "b", "S0" .., "W0" .., "c0" .."""
    loss, l2 = forward(H, V, b, S, layers, ptr, items, f, pid, pool, relu_last, w, off, scale)
    g = grads(H, V, b, S, layers, ptr, items, f, pid, pool, relu_last, w, off, scale, l2_reg, l2_mlp)
    if hasattr(opt, "begin_step"):
        opt.begin_step()
    if "history" in train and len(items):
        opt.apply(H, np.asarray(items), g["gh"], key="H")
    if "side" in train:
        for j, (Sj, fj) in enumerate(zip(S, f)):
            opt.apply(Sj, np.asarray(fj), g["gS"][j], key=f"S{j}")
    if "tower" in train:
        for l, (W, cl) in enumerate(layers):
            opt.apply_dense(W, g["dW"][l], key=f"W{l}")
            if cl is not None:
                opt.apply_dense(cl, g["dc"][l], key=f"c{l}")
    if "item" in train:
        opt.apply_dense(V, g["GV"], key="V")
    if b is not None and "bias" in train:
        opt.apply_dense(b, g["Gb"][:, None], key="b")
    return loss, l2
