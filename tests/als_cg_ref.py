"""NumPy reference of the conjugate-gradient ALS half-step (orx_als_half_step_cg) and of the ALS objective in its sparse form
(orx_als_objective).  With the notation of tests/als_ref.py, a row never forms A_r:

    A v  :=  b (G v) + reg v + sum_{j in O_r} (c_j - b) (f_j . v) f_j
    x = the row's current value;  r = y_r - A x;  p = r;  rs = r . r
    repeat cg_steps times:
        if rs <= 1e-20: the row is done, x stays
        Ap = A p;  alpha = rs / (p . Ap);  x += alpha p;  r -= alpha Ap
        rsn = r . r;  p = r + (rsn / rs) p;  rs = rsn

once in float64 (`cg64`) and once with every array and scalar in float32 (`cg32`: the yardstick against which the device's error
is held); `cg32_permuted` is a second float32 ordering of the same sums.  The objective by

    b <G_U, G_V>_F + sum_{(u,i) observed} [ c (1 - s)^2 - b s^2 ] + reg (|U|_F^2 + |V|_F^2),     s = u . v

in float64 and in float32, and `objective_bound`: the first-order forward bound of fp32 recursive summation under fp64 reductions."""
import numpy as np


def _cg(F, X, row_ptr, cols, conf, a, b, reg, steps, dtype, rows=None):
    F = np.asarray(F, dtype)
    X = np.array(X, dtype)
    a, b, reg = dtype(a), dtype(b), dtype(reg)
    G = (F.T @ F).astype(dtype)
    for r in (range(X.shape[0]) if rows is None else rows):
        o = np.asarray(cols[row_ptr[r]:row_ptr[r + 1]], np.int64)
        if o.size == 0:
            X[r] = 0
            continue
        c = np.full(o.size, a, dtype) if conf is None else np.asarray(conf[row_ptr[r]:row_ptr[r + 1]], dtype)
        Fo, w = F[o], (c - b).astype(dtype)

        def A(v):
            return (b * (G @ v) + reg * v + Fo.T @ (w * (Fo @ v))).astype(dtype)

        y = (Fo * c[:, None]).sum(axis=0).astype(dtype)
        x = X[r].copy()
        res = (y - A(x)).astype(dtype)
        p = res.copy()
        rs = dtype(res @ res)
        for _ in range(steps):
            if rs <= 1e-20:
                break
            Ap = A(p)
            alpha = dtype(rs / dtype(p @ Ap))
            x = (x + alpha * p).astype(dtype)
            res = (res - alpha * Ap).astype(dtype)
            rsn = dtype(res @ res)
            p = (res + dtype(rsn / rs) * p).astype(dtype)
            rs = rsn
        assert x.dtype == dtype and p.dtype == dtype
        X[r] = x
    return X


def cg64(F, X, row_ptr, cols, conf, a, b, reg, steps, rows=None):
    """float64: -> the new X (a copy; rows outside `rows` keep their values)"""
    return _cg(F, X, row_ptr, cols, conf, a, b, reg, steps, np.float64, rows)


def cg32(F, X, row_ptr, cols, conf, a, b, reg, steps, rows=None):
    """the same statements with every array and scalar in float32"""
    return _cg(F, X, row_ptr, cols, conf, a, b, reg, steps, np.float32, rows)


def cg32_permuted(F, X, row_ptr, cols, conf, a, b, reg, steps, seed=0):
    """cg32 over another ordering of every sum: the columns of F (and of X) permuted, the entries of each row reversed"""
    F, X = np.asarray(F, np.float32), np.asarray(X, np.float32)
    perm = np.random.default_rng(seed).permutation(F.shape[1])
    rcols, rconf = np.array(cols), None if conf is None else np.array(conf)
    for r in range(len(row_ptr) - 1):
        s = slice(row_ptr[r], row_ptr[r + 1])
        rcols[s] = rcols[s][::-1]
        if rconf is not None:
            rconf[s] = rconf[s][::-1]
    out = cg32(np.ascontiguousarray(F[:, perm]), np.ascontiguousarray(X[:, perm]), row_ptr, rcols, rconf, a, b, reg, steps)
    back = np.empty_like(out)
    back[:, perm] = out
    return back


def _objective(U, V, row_ptr, cols, conf, a, b, reg, dtype, absolute=False):
    U, V = np.asarray(U, dtype), np.asarray(V, dtype)
    if absolute:
        U, V = np.abs(U), np.abs(V)
    b, reg = dtype(b), dtype(reg)
    r = np.repeat(np.arange(U.shape[0]), np.diff(row_ptr))
    c = np.full(len(cols), a, dtype) if conf is None else np.asarray(conf, dtype)
    s = (U[r] * V[np.asarray(cols, np.int64)]).sum(axis=1).astype(dtype)
    one = dtype(1)
    obs = c * (one + s) ** 2 + b * s * s if absolute else c * (one - s) ** 2 - b * s * s
    gram = ((U.T @ U).astype(dtype) * (V.T @ V).astype(dtype)).sum(dtype=dtype)
    val = b * gram + obs.sum(dtype=dtype) + reg * ((U * U).sum(dtype=dtype) + (V * V).sum(dtype=dtype))
    assert np.asarray(val).dtype == dtype
    return val


def objective64(U, V, row_ptr, cols, conf, a, b, reg):
    """the sparse form in float64 (equal to als_ref.objective over the dense grid up to float64 rounding)"""
    return float(_objective(U, V, row_ptr, cols, conf, a, b, reg, np.float64))


def objective32(U, V, row_ptr, cols, conf, a, b, reg):
    """the same statements with every array and scalar in float32"""
    return float(_objective(U, V, row_ptr, cols, conf, a, b, reg, np.float32))


def objective_bound(U, V, row_ptr, cols, conf, a, b, reg):
    """(NU + NI + 2 D + 8) 2^-24 S, S the formula with every term replaced by its absolute value, float64"""
    S = float(_objective(U, V, row_ptr, cols, conf, a, b, reg, np.float64, absolute=True))
    return (U.shape[0] + V.shape[0] + 2 * U.shape[1] + 8) * 2.0 ** -24 * S
