"""Plain NumPy restatements of the fp16 MLP products (openrec_amd/csrc/kernels_gemm16.hip), in float64 on the fp16-rounded operands,
and the element-wise error bounds the device results are held to.

Two input regimes (tests/test_gpu_gemm16.py):

exact     operands, bias, Y, the initial C and out_scale are small integers or multiples of 1/4: every product and every partial sum,
          in ANY summation order, is a multiple of 2^-8 far below 2^24 of them -- representable in fp32 -- so a correct kernel returns the
          reference's bits and the tests assert equality.  test_gemm16_cpu.py proves the regime per case: the same reference in float32
          (NumPy's own summation order) equals the float64 one bit for bit.
rounding  normal / uniform operands of mixed magnitude.  A sum of K exact products (fp16 x fp16 is exact in fp32) accumulated in fp32 in any
          order, rounded or chopped, is within  K u (|A| |B|^T)_ij + u |ref_ij|,  u = 2^-23  (Higham, Accuracy and Stability, (3.5), with
          the unit roundoff of chopping).  Every further fp32 operation of an epilogue adds u |its result|; a sigmoid adds 4 ulp32 of the
          output (the device's exp and division).  Derived, not measured.
"""
import numpy as np

U = 2.0 ** -23
ACTS = {0: "none", 1: "relu", 2: "sigmoid"}


def act_fwd(v, act):
    if act == 1:
        return np.maximum(v, 0)
    if act == 2:
        return 1.0 / (1.0 + np.exp(-v))
    return v


def act_bwd(v, Y, act_y):
    """dZ = dX * act'(Y), Y the layer's OUTPUT (relu'(0) = 0)"""
    Y = Y.astype(v.dtype)
    if act_y == 1:
        return np.where(Y > 0, v, 0).astype(v.dtype)
    if act_y == 2:
        return v * Y * (1 - Y)
    return v


def nt(A, B, bias=None, act=0, Y=None, act_y=0, dtype=np.float64):
    """epilogue(A[M][K] B[N][K]^T): + bias, act, then the fused activation backward with Y"""
    v = A.astype(dtype) @ B.astype(dtype).T
    if bias is not None:
        v = v + bias.astype(dtype)[None, :]
    v = act_fwd(v, act)
    if Y is not None:
        v = act_bwd(v, Y, act_y)
    return v


def nt_bound(A, B, ref, bias=None, act=0, Y=None, act_y=0):
    """element-wise bound of the fp32 result against nt(...) in float64 (module docstring)"""
    A64, B64 = np.abs(A.astype(np.float64)), np.abs(B.astype(np.float64))
    K = A.shape[1]
    mag = A64 @ B64.T
    terms = K
    if bias is not None:                       # the bias is one more term of the sum
        mag = mag + np.abs(bias.astype(np.float64))[None, :]
        terms += 1
    pre = A.astype(np.float64) @ B.astype(np.float64).T + (0 if bias is None else bias.astype(np.float64)[None, :])
    b = terms * U * mag + U * np.abs(pre)
    if act == 2:                               # |sigmoid'| <= 1/4
        b = 0.25 * b + 4 * np.spacing(np.abs(act_fwd(pre, 2)).astype(np.float32)).astype(np.float64)
    if Y is not None and act_y == 2:           # v * y * (1 - y): the factor carried through, three more fp32 operations
        y = Y.astype(np.float64)
        b = b * np.abs(y * (1 - y)) * (1 + 4 * U) + 3 * U * np.abs(ref)
    return b


def colsums(dZ, block):
    """bias-gradient partial rows: row p = the column sums of rows [p * block, (p + 1) * block) -- the kernel stores one row per
    row block of its tile, the DLRM step adds them in row order"""
    M = dZ.shape[0]
    P = (M + block - 1) // block
    return np.stack([dZ[p * block:(p + 1) * block].sum(axis=0) for p in range(P)])


def colsum_bound(bound, dZ):
    """column sums over all rows: the elements' own bounds plus M fp32 additions of their magnitudes"""
    M = dZ.shape[0]
    return bound.sum(axis=0) + M * U * np.abs(dZ).sum(axis=0)


def tn(C0, A, B, out_scale, dtype=np.float64):
    """C0[M][N] + out_scale * A[K][M]^T B[K][N]"""
    return C0.astype(dtype) + dtype(out_scale) * (A.astype(dtype).T @ B.astype(dtype))


def tn_bound(C0, A, B, out_scale, ref):
    """K products in any order (slices, K groups, slab sums are all partial sums of the same terms), the scaling, the += into C"""
    K = A.shape[0]
    mag = np.abs(A.astype(np.float64)).T @ np.abs(B.astype(np.float64))
    prod = A.astype(np.float64).T @ B.astype(np.float64)
    return abs(out_scale) * (K * U * mag + 2 * U * np.abs(prod)) + U * np.abs(ref)


def head_fwd(X, w, bias, act, dtype=np.float64):
    return act_fwd(X.astype(dtype) @ w.astype(dtype) + dtype(bias), act)


def head_fwd_bound(X, w, bias, act):
    K = X.shape[1]
    mag = np.abs(X.astype(np.float64)) @ np.abs(w.astype(np.float64)) + abs(float(bias))
    pre = X.astype(np.float64) @ w.astype(np.float64) + float(bias)
    b = (K + 1) * U * mag + U * np.abs(pre)
    if act == 2:
        b = 0.25 * b + 4 * np.spacing(np.abs(act_fwd(pre, 2)).astype(np.float32)).astype(np.float64)
    return b


def head_bwd(X, w, dy, pred, act, act_below, dtype=np.float64):
    """dz = dy * act'(pred); its fp16 rounding dz16 is what the products use (the MFMA path rounds it there too):
    gb = sum dz; gW[k] = sum_b X[b][k] dz16[b]; dZ[b][k] = dz16[b] w[k] act_below'(X[b][k]); gb_below[k] = sum_b dZ[b][k]"""
    dz = act_bwd(dy.astype(dtype), pred, act)
    dz16 = dz.astype(np.float16).astype(dtype)
    gW = (X.astype(dtype) * dz16[:, None]).sum(axis=0)
    d = dz16[:, None] * w.astype(dtype)[None, :]
    dZ = act_bwd(d, X, act_below)
    return dict(gb=dz.sum(), gW=gW, dZ=dZ, gb_below=dZ.sum(axis=0))


def cast16(src, ld16):
    """[M][N] fp32 -> [M][ld16] fp16, round to nearest even (NumPy's conversion), overflow to inf; the columns from N on are zero"""
    M, N = src.shape
    out = np.zeros((M, ld16), np.float16)
    with np.errstate(over="ignore"):
        out[:, :N] = src.astype(np.float16)
    return out


def f16_interval(ref, bound):
    """the fp16 values a correct kernel may store: fp16 rounding is monotone, so any fp32 result within `bound` of `ref` rounds into
    [fp16(ref - bound), fp16(ref + bound)] -- one value (np.float16(ref)) unless ref sits within the bound of a rounding boundary"""
    with np.errstate(over="ignore"):
        return (ref - bound).astype(np.float16), (ref + bound).astype(np.float16)
