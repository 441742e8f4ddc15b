"""NumPy fp32 restatement of WARP's resolution rule (orx_sampler_pairwise_warp, kernels_warp.hip), shared by tests/test_warp_cpu.py
and tests/test_gpu_warp.py.  The stream is not restated: (u, p) and candidate c are tests/hardneg_ref.py's, or tests/proposal_ref.py's
when a proposal is set.

Candidate c violates iff (s_c + margin) > s_p: one rounded fp32 add, then a compare, so a NaN on either side never violates.
t = 1 + the smallest violating column, or 0; the negative is column t - 1 (column 0 when t = 0); the weight is table[t - 1], or
+0.0 when t = 0."""
import numpy as np

import hardneg_ref as hr
import proposal_ref as pr


def candidates(raw, NI, seed, g, T, proposal=None):
    """-> (u, p, cand[len(g), T]) of the samples g; proposal: None or (thr, alias)"""
    if proposal is None:
        return hr.candidates(raw, NI, seed, g, T)
    return pr.candidates(raw, NI, seed, g, T, *proposal)


def violates(pos_score, cand_score, margin):
    """bool [n, T]"""
    sp = np.asarray(pos_score, np.float32).reshape(-1, 1)
    sc = np.asarray(cand_score, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        lhs = sc + np.float32(margin)                    # fp32 + fp32 -> one rounded fp32 add
        assert lhs.dtype == np.float32
        return lhs > sp


def resolve(pos_score, cand_score, margin, table):
    """-> (t int32[n], column int64[n], weight float32[n])"""
    v = violates(pos_score, cand_score, margin)
    table = np.asarray(table, np.float32)
    assert v.ndim == 2 and table.shape == (v.shape[1],)
    found = v.any(axis=1)
    first = np.argmax(v, axis=1)
    t = np.where(found, first + 1, 0).astype(np.int32)
    column = np.where(found, first, 0)
    weight = np.where(found, table[column], np.float32(0.0)).astype(np.float32)
    return t, column, weight
