"""NumPy restatement of the full softmax with a label SET per sample (include/openrec_hip.h, orx_seqrec_full_sets_step /
orx_tower_sets_step), shared by tests/test_labelsets_cpu.py and tests/test_gpu_labelsets.py.  Everything runs at the dtype of the
tables it is given.

    sample i: query q_i, entries e in [lptr[i], lptr[i + 1]) with items j_e = litems[e] and weights t_e (1 without lw);  T_i = sum_e t_e
    s_ij, lse_i as tests/fullsoftmax_ref.py has them;   l_i = T_i lse_i - sum_e t_e s_{i,j_e}
    loss = (1/B) sum_i w_i l_i;   l2_loss = 1/2 (sum |the query side's rows|^2 + sum over entries |V[j_e]|^2)
    a_ij = c_i (T_i pi_ij - sum_{e: j_e = j} t_e),  c_i = w_i / B;   n_j = the number of entries with item j (not weighted)
    gq[i] = scale sum_j a_ij V[j] + l2_reg q_i;   GV[j] = scale sum_i a_ij q_i + l2_reg n_j V[j];   Gb[j] = scale sum_i a_ij
The SeqRec form pools the query rows with tests/seqrec_ref.py and the tower form runs tests/tower_ref.py's layers on them; the
steps hand the gradients to the oracle's optimizers exactly as fullsoftmax_ref.seq_step and tower_ref.step do."""
import numpy as np

import fullsoftmax_ref as fr
import seqrec_ref as sr

U32 = fr.U32


def set_weights(lptr, litems, lw, NI, dt):
    """-> Tm [B, NI] the summed weight of every (sample, item), T [B], n [NI] the entries per item, own [n_lab], t [n_lab]"""
    lptr = np.asarray(lptr, np.int64)
    B = len(lptr) - 1
    own = sr.owners(lptr)
    it = np.asarray(litems, np.int64)
    t = np.ones(len(it), dt) if lw is None else np.asarray(lw, dt)
    Tm = np.zeros((B, NI), dt)
    np.add.at(Tm, (own, it), t)
    T = np.zeros(B, dt)
    np.add.at(T, own, t)
    return Tm, T, np.bincount(it, minlength=NI).astype(dt), own, t


def row_losses_q(Q, V, b, lptr, litems, lw=None, off=None, scale=1.0):
    dt = Q.dtype
    s = fr.scores(Q, V, b, off, scale)
    _, T, _, own, t = set_weights(lptr, litems, lw, len(V), dt)
    sl = np.zeros(len(Q), dt)
    np.add.at(sl, own, t * s[own, np.asarray(litems, np.int64)])
    return T * fr._lse(s) - sl


def forward_q(Q, V, b, lptr, litems, lw=None, w=None, off=None, scale=1.0, X0=None):
    """-> (loss, l2_loss); X0: the rows whose squares are the query side's l2 part (None: Q itself)"""
    dt = Q.dtype
    l = row_losses_q(Q, V, b, lptr, litems, lw, off, scale)
    wv = np.ones_like(l) if w is None else np.asarray(w, dt)
    v = V[np.asarray(litems, np.int64)]
    X = Q if X0 is None else X0
    return (wv * l).sum() / dt.type(len(l)), dt.type(0.5) * ((X * X).sum() + (v * v).sum())


def grads_q(Q, V, b, lptr, litems, lw=None, w=None, off=None, scale=1.0, l2_reg=0.0):
    """-> dict(gu [B, D], GV [NI, D], Gb [NI])"""
    dt = Q.dtype
    B = len(Q)
    s = fr.scores(Q, V, b, off, scale)
    pi = np.exp(s - fr._lse(s)[:, None]).astype(dt)
    Tm, T, n, _, _ = set_weights(lptr, litems, lw, len(V), dt)
    c = (np.ones(B, dt) if w is None else np.asarray(w, dt)) / dt.type(B)
    a = c[:, None] * (T[:, None] * pi - Tm)
    sc, l2 = dt.type(scale), dt.type(l2_reg)
    return dict(gu=sc * (a @ V) + l2 * Q, GV=sc * (a.T @ Q) + (l2 * n)[:, None] * V, Gb=sc * a.sum(0))


def row_bound_q(Q, V, b, lptr, litems, lw=None, off=None, scale=1.0):
    """bound_i = sum_e t_e row_bound_q(q_i, label j_e) + (len_i + 2) u (T_i |lse_i| + sum_e t_e |s_{i,j_e}|): l_i is the t-weighted
    sum of len_i single-label losses, each inside the project's own bound, added in fp32.  Evaluated in float64."""
    lptr = np.asarray(lptr, np.int64)
    B = len(lptr) - 1
    it = np.asarray(litems, np.int64)
    Q64, V64 = Q.astype(np.float64), V.astype(np.float64)
    b64 = None if b is None else b.astype(np.float64)
    off64 = None if off is None else np.asarray(off, np.float64)
    s = fr.scores(Q64, V64, b64, off64, scale)
    lse = fr._lse(s)
    _, T, _, own, t = set_weights(lptr, it, lw, len(V), np.dtype(np.float64))
    # fullsoftmax_ref.row_bound_q per entry (sample own[e], label it[e]), from one [B, NI] pass instead of one row per entry
    D, NI = V.shape[1], V.shape[0]
    Tm = np.abs(Q64) @ np.abs(V64).T
    if b64 is not None:
        Tm = Tm + np.abs(b64[:, 0])[None, :]
    Tm = scale * Tm
    if off64 is not None:
        Tm = Tm + np.where(np.isfinite(off64), np.abs(off64), 0.0)[None, :]
    e = (D + 4) * U32 / (1.0 - (D + 4) * U32) * Tm
    per = e.max(1)[own] + e[own, it] + (2 * NI + 32) * U32 + 2 * U32 * (np.abs(lse)[own] + np.abs(s[own, it]))
    out = np.zeros(B)
    np.add.at(out, own, t * per)
    sabs = np.zeros(B)
    np.add.at(sabs, own, t * np.abs(s[own, it]))
    return out + (np.diff(lptr) + 2) * U32 * (T * np.abs(lse) + sabs)


# ---- the SeqRec form ---------------------------------------------------------------------------------------------------------------
def seq_forward(H, V, b, ptr, items, lptr, litems, pool, lw=None, w=None, off=None, scale=1.0):
    Q, _ = sr.pool_rows(H, ptr, items, pool)
    return forward_q(Q, V, b, lptr, litems, lw, w, off, scale)


def seq_row_losses(H, V, b, ptr, items, lptr, litems, pool, lw=None, off=None, scale=1.0):
    Q, _ = sr.pool_rows(H, ptr, items, pool)
    return row_losses_q(Q, V, b, lptr, litems, lw, off, scale)


def seq_row_bound(H, V, b, ptr, items, lptr, litems, pool, lw=None, off=None, scale=1.0):
    Q, _ = sr.pool_rows(H, ptr, items, pool)
    return row_bound_q(Q, V, b, lptr, litems, lw, off, scale)


def seq_step(H, V, b, ptr, items, lptr, litems, opt, pool, lw=None, w=None, off=None, scale=1.0, l2_reg=0.0,
             train=("history", "item", "bias"), keys=("H", "V", "b")):
    """One train step in place on (H, V, b); returns (loss, l2_loss) of the pre-step tables"""
    Q, c = sr.pool_rows(H, ptr, items, pool)
    loss, l2 = forward_q(Q, V, b, lptr, litems, lw, w, off, scale)
    g = grads_q(Q, V, b, lptr, litems, lw, w, off, scale, l2_reg)
    own = sr.owners(ptr)
    gh = (c[own, None] * g["gu"][own]).astype(H.dtype)
    if hasattr(opt, "begin_step"):
        opt.begin_step()
    if "history" in train and len(items):
        opt.apply(H, np.asarray(items), gh, key=keys[0])
    fr._apply_items(opt, V, b, g, train, keys)
    return loss, l2


# ---- the tower form ----------------------------------------------------------------------------------------------------------------
def tower_row_losses(H, V, b, S, layers, ptr, items, f, lptr, litems, pool, relu_last=True, lw=None, off=None, scale=1.0):
    import tower_ref as tr
    return row_losses_q(tr.queries(H, S, layers, ptr, items, f, pool, relu_last), V, b, lptr, litems, lw, off, scale)


def tower_row_bound(H, V, b, S, layers, ptr, items, f, lptr, litems, pool, relu_last=True, lw=None, off=None, scale=1.0):
    import tower_ref as tr
    return row_bound_q(tr.queries(H, S, layers, ptr, items, f, pool, relu_last), V, b, lptr, litems, lw, off, scale)


def tower_step(H, V, b, S, layers, ptr, items, f, lptr, litems, opt, pool, relu_last=True, lw=None, w=None, off=None, scale=1.0,
               l2_reg=0.0, l2_mlp=0.0, train=("history", "item", "bias", "side", "tower")):
    """tower_ref.step with the label sets in the objective; returns (loss, l2_loss) of the pre-step tables"""
    import tower_ref as tr
    dt = H.dtype
    x0, c, so = tr.input_rows(H, S, ptr, items, f, pool)
    xs, _ = tr.tower(x0, layers, relu_last)
    Q = xs[-1]
    loss, l2 = forward_q(Q, V, b, lptr, litems, lw, w, off, scale, X0=x0)
    g = grads_q(Q, V, b, lptr, litems, lw, w, off, scale, 0.0)["gu"]                   # (no l2 on the query itself)
    gi = grads_q(Q, V, b, lptr, litems, lw, w, off, scale, l2_reg)
    l2c, lm = dt.type(l2_reg), dt.type(l2_mlp)
    L = len(layers)
    dW, dc = [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        W, cl = layers[l]
        relu = l + 1 < L or relu_last
        gm = np.where(xs[l + 1] > 0, g, dt.type(0)) if relu else g
        dW[l] = xs[l].T @ gm + lm * W
        if cl is not None:
            dc[l] = gm.sum(0)[None, :] + lm * cl
        g = gm @ W.T
    g0 = (g + l2c * x0).astype(dt)
    own = sr.owners(ptr)
    gh = (c[own, None] * g0[own, so:]).astype(dt)
    if hasattr(opt, "begin_step"):
        opt.begin_step()
    if "history" in train and len(items):
        opt.apply(H, np.asarray(items), gh, key="H")
    if "side" in train:
        c0 = 0
        for j, (Sj, fj) in enumerate(zip(S, f)):
            opt.apply(Sj, np.asarray(fj), np.ascontiguousarray(g0[:, c0:c0 + Sj.shape[1]]), key=f"S{j}")
            c0 += Sj.shape[1]
    if "tower" in train:
        for l, (W, cl) in enumerate(layers):
            opt.apply_dense(W, dW[l], key=f"W{l}")
            if cl is not None:
                opt.apply_dense(cl, dc[l], key=f"c{l}")
    if "item" in train:
        opt.apply_dense(V, gi["GV"], key="V")
    if b is not None and "bias" in train:
        opt.apply_dense(b, gi["Gb"][:, None], key="b")
    return loss, l2
