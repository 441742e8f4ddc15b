"""Reference and checker for the all-item scorer (runtime.score_all_items), NumPy only.

    dot   out[q, j] =  U[uid[q]] . V[j]               (+ b[j])
    gmf   out[q, j] =  (U[uid[q]] * w) . V[j]         (+ b[j])
    l2    out[q, j] = -sum_k (U[uid[q], k] - V[j, k])^2  (+ b[j])     the DIRECT form, not the expanded one of the matrix-core kernel

Two ways to hold a device result against `reference`:

bounded  `check`: every element within `bound`, the worst case of ANY correct fp32 evaluation.  With u = 2^-24 and n = D + 4
         roundings per element -- one for GMF's premultiply, D for the accumulation in whatever order, three for the L2 combine
         and the bias add -- every computed term carries a factor (1 + d)^n, |d| <= u, so

             |got - exact| <= n u / (1 - n u) * S,      S = sum_k |u_k w_k v_k| + |b_j|                      (dot: w = 1, gmf)
                                                        S = |u|^2 + |v|^2 + 2 sum_k |u_k v_k| + |b_j|        (l2)

         The L2 sum covers both forms: the expanded one adds exactly these terms, and the direct one has
         (u_k - v_k)^2 <= u_k^2 + v_k^2 + 2 |u_k v_k| with two roundings on the difference and one on the square.  Nothing here
         is measured on a device.

exact    `exact_tables` draws small integers: for D <= 1024 every partial sum of every kind, in any order and in the expanded L2
         form too, is an integer below 2^17, so fp32 has no rounding at all and the check is np.array_equal with the reference
         cast to fp32.  This mode sees indexing, layout, tail, bias-offset and unwritten-element errors with no tolerance; the
         bounded mode sees precision loss, which small integers cannot show."""
import numpy as np

KINDS = ("dot", "l2", "gmf")
U24 = 2.0 ** -24


def _flat(x):
    return None if x is None else np.asarray(x, np.float64).reshape(-1)


def _rows(kind, U, w, uid):
    u = np.asarray(U, np.float64)[np.asarray(uid, np.int64)]
    return u * _flat(w)[None, :] if kind == "gmf" else u


def reference(kind, U, V, b, w, uid):
    """float64 scores [len(uid), NI]; b / w as [NI, 1] / [D, 1] tables or flat, b None for a model without item biases"""
    assert kind in KINDS
    u = _rows(kind, U, w, uid)
    v = np.asarray(V, np.float64)
    if kind == "l2":
        out = np.empty((u.shape[0], v.shape[0]), np.float64)
        for q in range(u.shape[0]):                 # one user at a time: the [n, NI, D] broadcast would not fit for the long tables
            d = v - u[q][None, :]
            out[q] = -np.einsum("jk,jk->j", d, d)
    else:
        out = u @ v.T
    if b is not None:
        out = out + _flat(b)[None, :]
    return out


def bound(kind, U, V, b, w, uid):
    """the per-element worst-case fp32 error, float64 [len(uid), NI] (module docstring)"""
    assert kind in KINDS
    au = np.abs(_rows(kind, U, w, uid))
    av = np.abs(np.asarray(V, np.float64))
    D = av.shape[1]
    S = au @ av.T
    if kind == "l2":
        S = 2.0 * S + (au * au).sum(1)[:, None] + (av * av).sum(1)[None, :]
    if b is not None:
        S = S + np.abs(_flat(b))[None, :]
    n = D + 4
    return n * U24 / (1.0 - n * U24) * S


def _worst(ratio, k=5):
    flat = np.argsort(np.where(np.isnan(ratio), np.inf, ratio), axis=None)[::-1][:k]
    return ", ".join("(q=%d, j=%d: %.3g x bound)" % (*np.unravel_index(i, ratio.shape), ratio.flat[i]) for i in flat)


def check(got, kind, U, V, b, w, uid, what=""):
    """shape, dtype, finiteness and |got - reference| <= bound at EVERY element.  Where the reference itself is not finite (a
    NaN row, an infinite bias) the element has to be non-finite too; what exactly it holds is the caller's to assert."""
    got = np.asarray(got)
    n, NI = len(uid), np.asarray(V).shape[0]
    assert got.shape == (n, NI), "%s %s: shape %s, expected %s" % (what, kind, got.shape, (n, NI))
    assert got.dtype == np.float32, "%s %s: dtype %s" % (what, kind, got.dtype)
    if got.size == 0:
        return
    with np.errstate(invalid="ignore", over="ignore"):
        ref = reference(kind, U, V, b, w, uid)
        bnd = bound(kind, U, V, b, w, uid)
    fin = np.isfinite(ref)
    bad = fin & ~np.isfinite(got)
    assert not bad.any(), "%s %s: %d non-finite elements where the reference is finite, first at (q, j) = %s" % (
        what, kind, int(bad.sum()), tuple(np.argwhere(bad)[0]))
    leak = ~fin & np.isfinite(got)
    assert not leak.any(), "%s %s: %d finite elements where the reference is not, first at (q, j) = %s" % (
        what, kind, int(leak.sum()), tuple(np.argwhere(leak)[0]))
    err = np.where(fin, np.abs(np.where(fin, got, 0.0).astype(np.float64) - np.where(fin, ref, 0.0)), 0.0)
    lim = np.where(fin, bnd, 0.0)
    over = err > lim
    if over.any():
        ratio = np.where(over, err / np.maximum(lim, np.finfo(np.float64).tiny), 0.0)
        raise AssertionError("%s %s: %d of %d elements beyond the fp32 bound; worst %s" % (what, kind, int(over.sum()), got.size, _worst(ratio)))


def exact_tables(rng, NU, NI, D):
    """small-integer tables as float32: U, V in [-3, 3], w [D, 1] in [-2, 2], b [NI, 1] in [-8, 8] -> (U, V, w, b)"""
    assert D <= 1024, "beyond D = 1024 the partial sums are no longer guaranteed exact in fp32"
    U = rng.integers(-3, 4, (NU, D)).astype(np.float32)
    V = rng.integers(-3, 4, (NI, D)).astype(np.float32)
    w = rng.integers(-2, 3, (D, 1)).astype(np.float32)
    b = rng.integers(-8, 9, (NI, 1)).astype(np.float32)
    return U, V, w, b


def check_exact(got, kind, U, V, b, w, uid, what=""):
    """for `exact_tables`: the device result IS the reference, bit for bit"""
    got = np.asarray(got)
    want = reference(kind, U, V, b, w, uid).astype(np.float32)
    assert got.shape == want.shape, "%s %s: shape %s, expected %s" % (what, kind, got.shape, want.shape)
    assert got.dtype == np.float32, "%s %s: dtype %s" % (what, kind, got.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(~(got == want))
        q, j = bad[0]
        raise AssertionError("%s %s: %d of %d elements differ from the exact result, first at (q=%d, j=%d): got %r, expected %r" % (
            what, kind, len(bad), got.size, q, j, float(got[q, j]), float(want[q, j])))
