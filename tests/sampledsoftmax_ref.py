"""Float64 NumPy restatement of the sampled softmax over a shared candidate list (include/openrec_hip.h,
orx_sampled_softmax_step / orx_seqrec_sampled_step), for tests/test_gpu_sampledsoftmax.py.

    s_i+ = scale (q_i . V[pid_i] + b[pid_i]) + pos_off_i
    s_ic = scale (q_i . V[cand_c] + b[cand_c]) + cand_off_c;  -inf when cand_c == pid_i and mask_hits, when cand_off_c == -inf,
           and for a candidate id outside the item table
    l_i = logsumexp(s_i+, s_i.) - s_i+;  loss = 1/B sum w_i l_i;  l2_loss = 1/2 sum (|q_i|^2 + |V[pid_i]|^2)
A sample whose `live` entry is False (a bad uid or pid) has c_i = 0 and contributes nothing."""
import numpy as np

import fullsoftmax_ref as fr

U32 = fr.U32


def _f64(x):
    return None if x is None else np.asarray(x, np.float64)


def scores(Q, V, b, pid, cand, cand_off=None, pos_off=None, scale=1.0, mask_hits=True):
    """-> s+ [B], s [B, S] with -inf at every removed entry"""
    Q, V, b = _f64(Q), _f64(V), _f64(b)
    pid, cand = np.asarray(pid), np.asarray(cand)
    ok = (cand >= 0) & (cand < len(V))
    cs = np.where(ok, cand, 0)
    bias = np.zeros(len(V)) if b is None else b[:, 0]
    sp = scale * ((Q * V[pid]).sum(1) + bias[pid]) + (0.0 if pos_off is None else _f64(pos_off))
    s = scale * (Q @ V[cs].T + bias[cs][None, :]) + (0.0 if cand_off is None else _f64(cand_off)[None, :])
    gone = ~ok[None, :] | (mask_hits & (cand[None, :] == pid[:, None]))
    return sp, np.where(gone, -np.inf, s)


def row_losses(Q, V, b, pid, cand, cand_off=None, pos_off=None, scale=1.0, mask_hits=True, live=None):
    sp, s = scores(Q, V, b, pid, cand, cand_off, pos_off, scale, mask_hits)
    m = np.maximum(sp, s.max(1, initial=-np.inf))
    l = m + np.log(np.exp(sp - m) + np.exp(s - m[:, None]).sum(1)) - sp
    return l if live is None else np.where(live, l, 0.0)


def forward(Q, V, b, pid, cand, w=None, live=None, **kw):
    """-> (loss, l2_loss)"""
    B = len(pid)
    live = np.ones(B, bool) if live is None else live
    l = row_losses(Q, V, b, pid, cand, live=live, **kw)
    wv = np.ones(B) if w is None else _f64(w)
    sq = (_f64(Q) ** 2).sum(1) + (_f64(V)[np.asarray(pid)] ** 2).sum(1)
    return (wv * l).sum() / B, 0.5 * (sq * live).sum()


def row_bound(Q, V, b, pid, cand, cand_off=None, pos_off=None, scale=1.0, mask_hits=True):
    """the bound on |l_i (fp32, any summation order) - l_i (exact)|: fullsoftmax_ref.row_bound_q of row i on the small item table
    V[[pid_i] + cand] with the label in column 0 -- row i's objective is exactly a full softmax over that table; a removed
    column is one whose offset is -inf"""
    pid, cand = np.asarray(pid), np.asarray(cand)
    S = len(cand)
    ok = (cand >= 0) & (cand < len(V))
    out = np.empty(len(pid))
    for i, p in enumerate(pid):
        rows = np.concatenate(([p], np.where(ok, cand, 0)))
        off = np.zeros(1 + S)
        off[0] = 0.0 if pos_off is None else pos_off[i]
        off[1:] = 0.0 if cand_off is None else cand_off
        off[1:][~ok | (mask_hits & (cand == p))] = -np.inf
        out[i] = fr.row_bound_q(Q[i:i + 1], V[rows], None if b is None else b[rows], [0], off, scale)[0]
    return out


def grads(Q, V, b, pid, cand, w=None, cand_off=None, pos_off=None, scale=1.0, mask_hits=True, l2_reg=0.0, live=None, rel=None):
    """-> dict(gq [B, D]; rows [B + S] = pid | cand; gV [B + S, D], gb [B + S] per entry) and, with rel [B] (the relative error
    allowed on row i's coefficients), tq / tV / tb: the same sums over absolute values weighted by rel -- the error a fp32
    evaluation may have in each element"""
    Q, V = _f64(Q), _f64(V)
    pid, cand = np.asarray(pid), np.asarray(cand)
    B, S = len(pid), len(cand)
    live = np.ones(B, bool) if live is None else live
    sp, s = scores(Q, V, b, pid, cand, cand_off, pos_off, scale, mask_hits)
    m = np.maximum(sp, s.max(1, initial=-np.inf))
    tot = np.exp(sp - m) + np.exp(s - m[:, None]).sum(1)
    c = np.where(live, np.ones(B) if w is None else _f64(w), 0.0) / B
    a = c[:, None] * np.exp(s - m[:, None]) / tot[:, None]
    ap = -a.sum(1)
    Vc, Vp, Ql = V[np.where((cand >= 0) & (cand < len(V)), cand, 0)], V[pid], Q * live[:, None]
    g = dict(rows=np.concatenate((np.where(live, pid, -1), cand)),
             gq=scale * (a @ Vc + ap[:, None] * Vp) + l2_reg * Ql,
             gV=np.concatenate((scale * ap[:, None] * Ql + l2_reg * Vp * live[:, None], scale * (a.T @ Ql))),
             gb=np.concatenate((scale * ap, scale * a.sum(0))))
    if rel is not None:
        ar, apr = a * rel[:, None], np.abs(ap) * rel
        g["tq"] = scale * (ar @ np.abs(Vc) + apr[:, None] * np.abs(Vp)) + 2 * U32 * np.abs(l2_reg * Ql)
        g["tV"] = np.concatenate((scale * apr[:, None] * np.abs(Ql) + 2 * U32 * np.abs(l2_reg * Vp), scale * (ar.T @ np.abs(Ql))))
        g["tb"] = np.concatenate((scale * apr, scale * ar.sum(0)))
    return g


def scatter(n, rows, x):
    """the sum of the entries x per table row (rows outside [0, n) dropped) -> [n, ...]"""
    out = np.zeros((n,) + x.shape[1:])
    keep = (rows >= 0) & (rows < n)
    np.add.at(out, rows[keep], x[keep])
    return out
