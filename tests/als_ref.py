"""NumPy reference of the ALS half-step of WRMF (Hu / Koren / Volinsky): every row of X solved in closed form with F fixed,

    G   = F^T F
    A_r = b G + sum_{j in O_r} (c_rj - b) f_j f_j^T + reg I
    y_r = sum_{j in O_r} c_rj f_j
    x_r = A_r^-1 y_r            (np.linalg.solve; a row without observations is zero)

in float64 (`half_step`), and the same statements in float32 throughout (`half_step32`): the yardstick against which the device's
error is held.  `objective` is what the two half-steps descend, over the dense grid."""
import numpy as np


def _half_step(F, X, row_ptr, cols, conf, a, b, reg, dtype, rows=None):
    F = np.asarray(F, dtype)
    X = np.array(X, dtype)
    D = F.shape[1]
    a, b, reg = dtype(a), dtype(b), dtype(reg)
    G = (F.T @ F).astype(dtype)
    eye = np.eye(D, dtype=dtype)
    for r in (range(X.shape[0]) if rows is None else rows):
        o = np.asarray(cols[row_ptr[r]:row_ptr[r + 1]], np.int64)
        if o.size == 0:
            X[r] = 0
            continue
        c = np.full(o.size, a, dtype) if conf is None else np.asarray(conf[row_ptr[r]:row_ptr[r + 1]], dtype)
        Fo = F[o]
        A = (b * G + (Fo * (c - b)[:, None]).T @ Fo + reg * eye).astype(dtype)
        y = (Fo * c[:, None]).sum(axis=0).astype(dtype)
        X[r] = np.linalg.solve(A, y)
        assert X.dtype == dtype
    return X


def half_step(F, X, row_ptr, cols, conf, a, b, reg, rows=None):
    """float64: -> the new X (a copy; rows outside `rows` keep their values)"""
    return _half_step(F, X, row_ptr, cols, conf, a, b, reg, np.float64, rows)


def half_step32(F, X, row_ptr, cols, conf, a, b, reg, rows=None):
    """the same statements with every array and scalar in float32"""
    return _half_step(F, X, row_ptr, cols, conf, a, b, reg, np.float32, rows)


def dense_conf(row_ptr, cols, conf, a, b, shape):
    """-> (C, P) float64 [R, M]: the confidence and the preference of every cell"""
    C = np.full(shape, float(b), np.float64)
    P = np.zeros(shape, np.float64)
    r = np.repeat(np.arange(shape[0]), np.diff(row_ptr))
    C[r, cols] = float(a) if conf is None else np.asarray(conf, np.float64)
    P[r, cols] = 1.0
    return C, P


def objective(U, V, C, P, reg):
    """sum over all cells C (P - U V^T)^2 + reg (|U|_F^2 + |V|_F^2), float64"""
    U, V = np.asarray(U, np.float64), np.asarray(V, np.float64)
    E = P - U @ V.T
    return float((C * E * E).sum() + reg * ((U * U).sum() + (V * V).sum()))


def gradient_X(F, X, C, P, reg):
    """d objective / d X for the half-step with F fixed (C, P oriented [rows of X, rows of F]), float64"""
    F, X = np.asarray(F, np.float64), np.asarray(X, np.float64)
    return -2.0 * (C * (P - X @ F.T)) @ F + 2.0 * reg * X


def err_vs(x, x64):
    """max |x - x64| / max |x64|"""
    x64 = np.asarray(x64, np.float64)
    return float(np.abs(np.asarray(x, np.float64) - x64).max() / np.abs(x64).max())
