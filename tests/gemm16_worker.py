"""Runners of tests/test_gpu_gemm16.py: each takes one row of that module's case tables, calls the fp16 product entry points
(include/openrec_hip.h, "the fp16 MLP products alone") on torch-allocated device buffers and compares with tests/gemm16_ref.py.

Buffers.  Every output is surrounded by guards filled with a NaN bit pattern -- rows beyond M, columns between N and the leading
dimension, slab floats beyond the plan, mask words beyond the plan's -- and the guards must come back untouched.  Operand rows the
kernels never read (beyond M / N / the samples) are NaN.  The operands' padding columns (between K and lda for the nt product, between
M / N and lda / ldb for the tn product) are ZERO: that is the contract (the kernels multiply whole 16-byte chunks).
Every case runs twice; the two results must have the same bits.

As a program: `python gemm16_worker.py <set>` runs the cases of test_gpu_gemm16.ENV_SETS[<set>] under the environment the parent gave
this process (the ORX_GEMM16_* switches are read once per process) and prints one line per case."""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import gemm16_ref as ref  # noqa: E402

PAT32, PAT16, PAT64 = 0x7FC0DEAD, 0x7E5A, 0x7FF8DEADBEEF1234
SLAB_STRIDE = 128 * 128 + 64
GUARD_ROWS = 3


def up(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ plan queries (no device)
def plan(num_cu, M, N, K, lda, ldb):
    from openrec_amd import _ffi
    lib = _ffi.load()
    a, b = (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 8)()
    _ffi.check(lib.orx_gemm16_plan(num_cu, M, N, K, lda, ldb, a, b))
    nt = dict(zip(("cfg", "stages", "tail", "wave_tile", "bm", "bn", "blocks", "mask_words"), list(a)))
    tn = dict(zip(("S", "tiles", "kchunk", "form", "tail"), list(b)[:5]))
    return nt, tn


def group_plan(num_cu, B, in_, out, ldx, lddz, ldw, nt_cols=0):
    from openrec_amd import _ffi
    lib = _ffi.load()
    a = (ctypes.c_int32 * 8)()
    _ffi.check(lib.orx_gemm16_group_query(num_cu, B, in_, out, ldx, lddz, ldw, nt_cols, a))
    return dict(zip(("grouped", "tn_tail", "nt_tail", "S", "tiles", "kchunk", "n_tn", "n_nt"), list(a)))


# ------------------------------------------------------------------------------------------------ case data (host, NumPy only)
def draw(rng, shape, regime, kind="operand"):
    """exact: integers in -3 .. 3 (sigmoid outputs: multiples of 1/4 in [0, 1]); rounding: normal values times 2^(-3 .. 2)"""
    if kind == "sig_y":
        if regime == "exact":
            return rng.integers(0, 5, shape) / 4.0
        return rng.uniform(0.0, 1.0, shape)
    if regime == "exact":
        return rng.integers(-3, 4, shape).astype(np.float64)
    v = rng.standard_normal(shape) * 2.0 ** rng.integers(-3, 3, shape)
    if kind == "relu_y":                                  # a relu layer's output: exact zeros
        v = np.where(rng.uniform(size=shape) < 0.3, 0.0, np.abs(v))
    return v


def operand16(rng, rows, cols, ld, regime, kind="operand", extra_zero_rows=0):
    """[rows + guards][ld] fp16: the used block, zero padding columns, `extra_zero_rows` rows of zeros, then NaN rows nobody reads"""
    a = np.full((rows + extra_zero_rows + GUARD_ROWS, ld), np.nan, np.float16)
    a[:rows + extra_zero_rows] = 0
    a[:rows, :cols] = draw(rng, (rows, cols), regime, kind).astype(np.float16)
    return a


def nt_layout(c):
    M, N, K = c["M"], c["N"], c["K"]
    lda = up(K, c.get("pad", 8))
    return M, N, K, lda, lda


def nt_host(c):
    """operands and float64 reference of an nt case (the mask form's Y comes from the device: see run_nt)"""
    M, N, K, lda, ldb = nt_layout(c)
    rng = np.random.default_rng(c.get("seed", 1) + 1000003 * M + 1009 * N + K)
    regime = c.get("regime", "exact")
    h = dict(A=operand16(rng, M, K, lda, regime), B=operand16(rng, N, K, ldb, regime), bias=None, Y=None)
    if c.get("bias"):
        h["bias"] = draw(rng, (N,), regime).astype(np.float32)
    y = c.get("y")
    if y in ("f32", "f16"):
        ydt = np.float32 if y == "f32" else np.float16
        h["Y"] = draw(rng, (M, N), regime, "sig_y" if c.get("act_y") == 2 else "relu_y").astype(ydt)
    return h


def mask_layer_host(M, N, regime):
    """operands of the relu layer below a "mask" case: its forward launch [M][N] = relu(A2 B2^T) writes the fp16 output and the mask"""
    rng = np.random.default_rng(99 + M + N)
    return operand16(rng, M, 64, 64, regime), operand16(rng, N, 64, 64, regime)


def nt_reference(c, h, dtype=np.float64):
    M, N, K = c["M"], c["N"], c["K"]
    return ref.nt(h["A"][:M, :K], h["B"][:N, :K], h["bias"], c.get("act", 0), h["Y"], c.get("act_y", 0), dtype=dtype)


def tn_host(c):
    M, N, K = c["M"], c["N"], c["K"]
    lda, ldb = c.get("lda", up(M, 128)), c.get("ldb", up(N, 128))
    rng = np.random.default_rng(c.get("seed", 2) + 1000003 * M + 1009 * N + K)
    regime = c.get("regime", "exact")
    return dict(A=operand16(rng, K, M, lda, regime), B=operand16(rng, K, N, ldb, regime),
                C0=draw(rng, (M, N), regime).astype(np.float32), lda=lda, ldb=ldb)


def tn_reference(c, h, dtype=np.float64):
    M, N, K = c["M"], c["N"], c["K"]
    return ref.tn(h["C0"], h["A"][:K, :M], h["B"][:K, :N], c.get("scale", 1.0), dtype=dtype)


def head_host(c):
    B, K = c["B"], c["K"]
    ldx = up(K, c.get("pad", 8))
    rng = np.random.default_rng(c.get("seed", 3) + 1009 * B + K)
    regime = c.get("regime", "exact")
    act, below = c.get("act", 0), c.get("below", 0)
    h = dict(X=operand16(rng, B, K, ldx, regime, "sig_y" if below == 2 else "operand"), ldx=ldx,
             w=draw(rng, (up(K, 8),), regime).astype(np.float16), bias=np.float32(draw(rng, (), regime)))
    h["w"][K:] = 0
    h["dy"] = draw(rng, (B,), "exact").astype(np.float32)
    h["pred"] = draw(rng, (B,), "exact", "sig_y" if act == 2 else "operand").astype(np.float32)
    return h


# ------------------------------------------------------------------------------------------------ device side
class Dev:
    """torch allocations, the library's context, the calls"""

    def __init__(self):
        import torch
        from openrec_amd import _ffi, runtime as rt
        self.torch, self.ffi, self.lib = torch, _ffi, _ffi.load()
        self.ctx = rt.Context(0)
        self.num_cu = torch.cuda.get_device_properties(0).multi_processor_count
        self.stats = {}

    def put(self, a):
        if a is None:
            return None
        t = self.torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return t

    def guarded(self, rows, ld, bits):
        """[rows + guards][ld] of the NaN pattern, as a device tensor of the unsigned type of that width"""
        dt, pat = {32: (np.int32, PAT32), 16: (np.int16, PAT16), 64: (np.int64, PAT64)}[bits]
        return self.put(np.full((rows + GUARD_ROWS, ld), pat, dt))

    def ptr(self, t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def ready(self):
        self.ctx.wait_stream(self.torch.cuda.current_stream().cuda_stream)

    def get(self, t, dtype):
        return t.cpu().numpy().view(dtype)

    def record(self, kernel, ratio):
        self.stats[kernel] = max(self.stats.get(kernel, 0.0), float(ratio))


def check_guards(bits, rows, cols, pat, what):
    """bits: [rows + guards][ld] raw words after the call"""
    assert (bits[rows:] == pat).all(), f"{what}: rows beyond {rows} were written"
    assert (bits[:rows, cols:] == pat).all(), f"{what}: columns between {cols} and the leading dimension {bits.shape[1]} were written"


def check_values(got, want, bound, what, dev=None, kernel=None):
    """exact regime (bound None): bit equality (with -0 == +0: a relu backward's 0 may carry the product's sign)"""
    if bound is None:
        bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
        assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ from the exact reference, first at {tuple(np.argwhere(bad)[0])}: " \
                              f"{got[tuple(np.argwhere(bad)[0])]!r} != {want[tuple(np.argwhere(bad)[0])]!r}"
        return
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    if dev is not None and kernel:
        dev.record(kernel, ratio)
    print(f"    {what}: worst error / bound {ratio:.3g}")
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} elements beyond the derived bound, worst {ratio:.3g} x"


def check_f16(got16, want, bound, what):
    """the fp16 copy: np.float16(ref), or within the interval the fp32 bound allows around a rounding boundary"""
    if bound is None:
        with np.errstate(over="ignore"):
            w16 = want.astype(np.float16)
        bad = ~((got16 == w16) | (np.isnan(got16) & np.isnan(w16)))
        assert not bad.any(), f"{what}: {int(bad.sum())} fp16 elements differ from np.float16(reference), first at {tuple(np.argwhere(bad)[0])}"
        return
    lo, hi = ref.f16_interval(want, bound)
    bad = ~((got16 >= lo) & (got16 <= hi))
    assert not bad.any(), f"{what}: {int(bad.sum())} fp16 elements outside [fp16(ref - bound), fp16(ref + bound)]"


def nt_call(d, A, lda, B, ldb, M, N, K, out, ldc, ldc16, bias=None, act=0, Y=None, ykind=None, ldy=0, act_y=0, colsum=False,
            mask_words=0, mask_in=None, expect=0):
    """one launch into fresh guarded outputs; returns the raw words of everything it may have written"""
    C = d.guarded(M, ldc, 32) if out in ("C", "both") else None
    C16 = d.guarded(M, ldc16, 16) if out in ("C16", "both") else None
    pmax = (M + 127) // 128
    parts = d.guarded(pmax, N, 32) if colsum else None
    mask = d.guarded(1, mask_words, 64) if mask_words else None      # (row 0: the words; the guard rows: words beyond the plan)
    P = ctypes.c_int32(-1)
    d.ready()
    rc = d.lib.orx_gemm16_nt(d.ctx._h, d.ptr(A), lda, d.ptr(B), ldb, d.ptr(C), ldc, d.ptr(C16), ldc16, d.ptr(bias), M, N, K, act,
                             d.ptr(Y) if ykind == "f32" else None, d.ptr(Y) if ykind == "f16" else None, ldy, act_y,
                             d.ptr(parts), ctypes.byref(P), d.ptr(mask), d.ptr(mask_in))
    if expect != 0:
        assert rc == expect, f"expected return code {expect}, got {rc}"
        d.ctx.synchronize()
        return None
    d.ffi.check(rc)
    d.ctx.synchronize()
    r = dict(P=P.value, mask_t=mask)
    r["C"] = d.get(C, np.uint32) if C is not None else None
    r["C16"] = d.get(C16, np.uint16) if C16 is not None else None
    r["parts"] = d.get(parts, np.uint32) if parts is not None else None
    r["mask"] = d.get(mask, np.uint64) if mask is not None else None
    return r


def same_bits(a, b, what):
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), f"{what}: {k} differs between two runs of the same call ({int((a[k] != b[k]).sum())} words)"
    assert a.get("P") == b.get("P")


def check_nt_result(d, c, r, want, bound, M, N, block, what, kernel):
    if r["C"] is not None:
        check_guards(r["C"], M, N, PAT32, what + " C")
        check_values(r["C"][:M, :N].view(np.float32), want, bound, what + " C", d, kernel)
    if r["C16"] is not None:
        check_guards(r["C16"], M, N, PAT16, what + " C16")
        check_f16(r["C16"][:M, :N].view(np.float16), want, bound, what + " C16")
    if r["parts"] is not None:
        P = (M + block - 1) // block
        assert r["P"] == P, f"{what}: P = {r['P']}, expected ceil({M} / {block}) = {P}"
        check_guards(r["parts"], P, N, PAT32, what + " column sums")
        got = r["parts"][:P, :N].view(np.float32)
        if bound is None:
            check_values(got, ref.colsums(want, block), None, what + " column-sum partial rows")
        check_values(got.astype(np.float64).sum(axis=0), want.sum(axis=0), None if bound is None else ref.colsum_bound(bound, want),
                     what + " column sums", d, kernel + "_colsum")


def run_nt(d, c):
    """forward or backward epilogue of the nt product, per the case row"""
    M, N, K, lda, ldb = nt_layout(c)
    what = "nt " + c["id"]
    h = nt_host(c)
    regime = c.get("regime", "exact")
    p, _ = plan(d.num_cu, M, N, K, lda, ldb)
    out = c.get("out", "both")
    ldc, ldc16 = N + c.get("ldc_extra", 4), N + c.get("ldc16_extra", 8)
    A, B, bias = d.put(h["A"]), d.put(h["B"]), d.put(h["bias"])
    ykind, ldy, Y = c.get("y"), N + c.get("ldy_extra", 8), None
    mask_in = None
    if ykind == "mask":
        # the layer below: a relu forward of the same [M][N] leaves its fp16 output and the mask of "output > 0"
        A2, B2 = mask_layer_host(M, N, regime)
        assert p["mask_words"] > 0
        f1 = nt_call(d, d.put(A2), 64, d.put(B2), 64, M, N, 64, "C16", 0, ldy, act=1, mask_words=p["mask_words"])
        f2 = nt_call(d, d.put(A2), 64, d.put(B2), 64, M, N, 64, "C16", 0, ldy, act=1, mask_words=p["mask_words"])
        same_bits({k: v for k, v in f1.items() if k != "mask_t"}, {k: v for k, v in f2.items() if k != "mask_t"}, what + " (mask forward)")
        assert (f1["mask"][1:] == PAT64).all(), f"{what}: mask words beyond the plan's {p['mask_words']} were written"
        check_guards(f1["C16"], M, N, PAT16, what + " (mask forward) C16")
        want_y = ref.nt(A2[:M], B2[:N], act=1)
        check_f16(f1["C16"][:M, :N].view(np.float16), want_y, None if regime == "exact" else ref.nt_bound(A2[:M], B2[:N], want_y), what + " (mask forward)")
        h["Y"] = f1["C16"][:M, :N].view(np.float16).copy()
        assert (h["Y"] == 0).any() and (h["Y"] > 0).any()
        ybuf = np.full((M + GUARD_ROWS, ldy), np.nan, np.float16); ybuf[:M, :N] = h["Y"]
        Y, ykind, mask_in = d.put(ybuf), "f16", f1["mask_t"]
    elif ykind in ("f32", "f16"):
        ybuf = np.full((M + GUARD_ROWS, ldy), np.nan, h["Y"].dtype); ybuf[:M, :N] = h["Y"]
        Y = d.put(ybuf)
    want = nt_reference(c, h)
    bound = None if regime == "exact" else ref.nt_bound(h["A"][:M, :K], h["B"][:N, :K], want, h["bias"], c.get("act", 0), h["Y"], c.get("act_y", 0))
    kw = dict(bias=bias, act=c.get("act", 0), Y=Y, ykind=ykind, ldy=ldy, act_y=c.get("act_y", 0), colsum=bool(c.get("colsum")))
    mw = p["mask_words"] if c.get("mask_out") else 0
    r1 = nt_call(d, A, lda, B, ldb, M, N, K, out, ldc, ldc16, mask_words=mw, **kw)
    r2 = nt_call(d, A, lda, B, ldb, M, N, K, out, ldc, ldc16, mask_words=mw, **kw)
    strip = lambda r: {k: v for k, v in r.items() if k != "mask_t"}      # noqa: E731
    same_bits(strip(r1), strip(r2), what)
    kernel = f"nt_cfg{p['cfg']}"
    check_nt_result(d, c, r1, want, bound, M, N, p["bm"], what, kernel)
    if mw:
        assert (r1["mask"][1:] == PAT64).all(), f"{what}: mask words beyond the plan's {mw} were written"
    if mask_in is not None:
        r3 = nt_call(d, A, lda, B, ldb, M, N, K, out, ldc, ldc16, mask_in=mask_in, **kw)
        same_bits(strip(r1), strip(r3), what + ": backward with mask_in against backward with actY16")
    if mw and c.get("act", 0) == 1 and out != "C":
        # a mask written here serves a backward launch of the same shape: same result as with the fp16 output itself
        rngb = np.random.default_rng(7 + M)
        A3, B3 = operand16(rngb, M, 64, 64, "exact"), operand16(rngb, N, 64, 64, "exact")
        ycopy = np.full((M + GUARD_ROWS, ldc16), np.nan, np.float16); ycopy[:M, :N] = r1["C16"][:M, :N].view(np.float16)
        Yd = d.put(ycopy)
        kwb = dict(Y=Yd, ykind="f16", ldy=ldc16, act_y=1, colsum=True)
        b1 = nt_call(d, d.put(A3), 64, d.put(B3), 64, M, N, 64, "both", ldc, ldc16, **kwb)
        b2 = nt_call(d, d.put(A3), 64, d.put(B3), 64, M, N, 64, "both", ldc, ldc16, mask_in=r1["mask_t"], **kwb)
        same_bits(strip(b1), strip(b2), what + ": backward with the mask this forward wrote against backward with its fp16 output")
        wantb = ref.nt(A3[:M], B3[:N], Y=r1["C16"][:M, :N].view(np.float16), act_y=1)
        check_nt_result(d, c, b1, wantb, None, M, N, p["bm"], what + " (backward after the mask)", kernel)
    return p


def tn_call(d, A, lda, B, ldb, C0, ldc, slab, M, N, K, scale, expect=0):
    Cbuf = np.full((M + GUARD_ROWS, ldc), PAT32, np.uint32)
    Cbuf[:M, :N] = C0.view(np.uint32)
    C = d.put(Cbuf.view(np.int32))
    d.ready()
    rc = d.lib.orx_gemm16_tn(d.ctx._h, d.ptr(A), lda, d.ptr(B), ldb, d.ptr(C), ldc, d.ptr(slab), M, N, K, scale)
    if expect != 0:
        assert rc == expect, f"expected return code {expect}, got {rc}"
        d.ctx.synchronize()
        return None
    d.ffi.check(rc)
    d.ctx.synchronize()
    return dict(C=d.get(C, np.uint32))


def make_slab(d, tiles, S):
    n = tiles * S * SLAB_STRIDE if S > 1 else 0
    return d.put(np.full(n + 256, PAT32, np.uint32).view(np.int32)), n


def run_tn(d, c):
    """C += out_scale * A^T B from a non-zero C; `then` = batch sizes of further calls that reuse the same slab workspace as it stands"""
    M, N = c["M"], c["N"]
    what = "tn " + c["id"]
    regime = c.get("regime", "exact")
    ldc = N + c.get("ldc_extra", 4)
    slab, p0 = None, None
    for K in [c["K"]] + list(c.get("then", ())):
        cc = dict(c, K=K)
        h = tn_host(cc)
        _, p = plan(d.num_cu, M, N, K, h["lda"], h["ldb"])
        if slab is None:
            slab, slab_n = make_slab(d, p["tiles"], p["S"])
            p0 = p
        assert (p["S"], p["tiles"]) == (p0["S"], p0["tiles"]), "the split depends on the gradient's shape only"
        A, B = d.put(h["A"]), d.put(h["B"])
        scale = c.get("scale", 1.0)
        r1 = tn_call(d, A, h["lda"], B, h["ldb"], h["C0"], ldc, slab, M, N, K, scale)
        r2 = tn_call(d, A, h["lda"], B, h["ldb"], h["C0"], ldc, slab, M, N, K, scale)
        same_bits(r1, r2, f"{what} K={K}")
        want = tn_reference(cc, h)
        bound = None if regime == "exact" else ref.tn_bound(h["C0"], h["A"][:K, :M], h["B"][:K, :N], scale, want)
        check_guards(r1["C"], M, N, PAT32, f"{what} K={K} C")
        check_values(r1["C"][:M, :N].view(np.float32), want, bound, f"{what} K={K}", d, f"tn_form{p['form']}")
        tail = d.get(slab, np.uint32)[slab_n:]
        assert (tail == PAT32).all(), f"{what} K={K}: slab floats beyond the plan's tiles * S * stride were written"
    return p0


def run_group(d, c):
    """the grouped launch against the two separate launches (bit for bit in the exact regime) and against the references"""
    B, in_, out = c["B"], c["in"], c["out"]
    what = "group " + c["id"]
    regime = c.get("regime", "exact")
    ldx, lddz, ldw = c["ldx"], c["lddz"], c["ldw"]
    nt_cols = c.get("nt_cols", 0)
    in_nt = nt_cols or in_
    rng = np.random.default_rng(c.get("seed", 5) + B + in_ + out)
    X, dZ = operand16(rng, B, in_, ldx, regime), operand16(rng, B, out, lddz, regime)
    W = operand16(rng, in_, out, ldw, regime, extra_zero_rows=in_nt - in_)           # (rows in .. nt_cols - 1: the operand's zero padding rows)
    C0 = draw(rng, (in_, out), regime).astype(np.float32)
    act_y = c.get("act_y", 1)
    Yh = draw(rng, (B, in_nt), regime, "sig_y" if act_y == 2 else "relu_y").astype(np.float16) if c.get("y", True) else None
    ldy = in_nt + 8
    Yd = None
    if Yh is not None:
        ybuf = np.full((B + GUARD_ROWS, ldy), np.nan, np.float16); ybuf[:B, :in_nt] = Yh
        Yd = d.put(ybuf)
    g = group_plan(d.num_cu, B, in_, out, ldx, lddz, ldw, nt_cols)
    assert (g["tn_tail"], g["nt_tail"]) == tuple(c["tails"]), f"{what}: the case was written for tails {c['tails']}, the plan says {g}"
    Xd, dZd, Wd = d.put(X), d.put(dZ), d.put(W)
    ldgw, ldc, ldc16 = out + 4, in_nt + 4, in_nt + 8
    scale = c.get("scale", 1.0)
    slab, slab_n = make_slab(d, g["tiles"], g["S"])

    def call():
        gWb = np.full((in_ + GUARD_ROWS, ldgw), PAT32, np.uint32); gWb[:in_, :out] = C0.view(np.uint32)
        gW = d.put(gWb.view(np.int32))
        C, C16 = d.guarded(B, ldc, 32), d.guarded(B, ldc16, 16)
        parts = d.guarded((B + 127) // 128, in_nt, 32) if Yd is not None else None
        P = ctypes.c_int32(-1)
        d.ready()
        d.ffi.check(d.lib.orx_gemm16_group(d.ctx._h, d.ptr(Xd), ldx, d.ptr(dZd), lddz, d.ptr(gW), ldgw, d.ptr(slab), in_, out, B, scale,
                                           d.ptr(Wd), ldw, d.ptr(C), ldc, d.ptr(C16), ldc16, None, d.ptr(Yd), ldy, act_y if Yd is not None else 0,
                                           d.ptr(parts), ctypes.byref(P), None, nt_cols))
        d.ctx.synchronize()
        return dict(gW=d.get(gW, np.uint32), C=d.get(C, np.uint32), C16=d.get(C16, np.uint16), P=P.value,
                    parts=d.get(parts, np.uint32) if parts is not None else None)

    r1, r2 = call(), call()
    same_bits(r1, r2, what)
    assert (d.get(slab, np.uint32)[slab_n:] == PAT32).all(), f"{what}: slab floats beyond the plan were written"
    want_w = ref.tn(C0, X[:B, :in_], dZ[:B, :out], scale)
    want_x = ref.nt(dZ[:B, :out], W[:in_nt, :out], Y=Yh, act_y=act_y if Yh is not None else 0)
    bw = None if regime == "exact" else ref.tn_bound(C0, X[:B, :in_], dZ[:B, :out], scale, want_w)
    bx = None if regime == "exact" else ref.nt_bound(dZ[:B, :out], W[:in_nt, :out], want_x, Y=Yh, act_y=act_y)
    check_guards(r1["gW"], in_, out, PAT32, what + " gW")
    check_values(r1["gW"][:in_, :out].view(np.float32), want_w, bw, what + " gW", d, "group_tn")
    check_nt_result(d, c, r1, want_x, bx, B, in_nt, 128, what + " dX", "group_nt")
    if nt_cols > in_:
        assert (r1["C"][:B, in_:in_nt] & 0x7FFFFFFF == 0).all(), f"{what}: the input gradient's padding columns are not zero"
    if regime == "exact":
        # the separate launches: other kernels (the two-K-group weight gradient), other summation orders -- the same bits here
        slab2, _ = make_slab(d, g["tiles"], g["S"])
        t = tn_call(d, Xd, ldx, dZd, lddz, C0, ldgw, slab2, in_, out, B, scale)
        assert np.array_equal(t["C"], r1["gW"]), f"{what}: the grouped weight gradient differs from orx_gemm16_tn's"
        n = nt_call(d, dZd, lddz, Wd, ldw, B, in_nt, out, "both", ldc, ldc16, Y=Yd, ykind="f16" if Yd is not None else None, ldy=ldy,
                    act_y=act_y if Yd is not None else 0, colsum=Yd is not None)
        pn, _ = plan(d.num_cu, B, in_nt, out, lddz, ldw)
        for k in ("C", "C16") + (("parts",) if pn["bm"] == 128 else ()):
            if r1[k] is not None:
                assert np.array_equal(n[k], r1[k]), f"{what}: the grouped input gradient's {k} differs from orx_gemm16_nt's"
    return g


def run_head_fwd(d, c):
    B, K = c["B"], c["K"]
    what = "head_fwd " + c["id"]
    regime = c.get("regime", "exact")
    h = head_host(c)
    X, w, bias = d.put(h["X"]), d.put(h["w"]), d.put(np.array([h["bias"]], np.float32))
    res = []
    for _ in range(2):
        pred = d.guarded(1, B + 5, 32)          # (row 0 holds pred[0 .. B) and five guard words)
        d.ready()
        d.ffi.check(d.lib.orx_head16_fwd(d.ctx._h, d.ptr(X), h["ldx"], d.ptr(w), d.ptr(bias), c.get("act", 0), d.ptr(pred), B, K))
        d.ctx.synchronize()
        res.append(d.get(pred, np.uint32))
    assert np.array_equal(res[0], res[1]), f"{what}: two runs differ"
    r = res[0]
    assert (r[0, B:] == PAT32).all() and (r[1:] == PAT32).all(), f"{what}: words beyond pred[B) were written"
    want = ref.head_fwd(h["X"][:B, :K], h["w"][:K], h["bias"], c.get("act", 0))
    bound = None if regime == "exact" else ref.head_fwd_bound(h["X"][:B, :K], h["w"][:K], h["bias"], c.get("act", 0))
    check_values(r[0, :B].view(np.float32), want, bound, what, d, "head_fwd")


def run_head_bwd(d, c):
    """exact regime only: pred and dy are inputs, so sigmoid' (multiples of 1/16) is exact as well"""
    B, K = c["B"], c["K"]
    what = "head_bwd " + c["id"]
    h = head_host(c)
    act, below = c.get("act", 0), c.get("below", 0)
    ld16, ld32 = up(K, 8) + 8, K + 3
    X, w, dy, pred = d.put(h["X"]), d.put(h["w"]), d.put(h["dy"]), d.put(h["pred"])
    blocks = d.lib.orx_head16_bwd_blocks(d.ctx._h, B)
    assert blocks >= 1
    res = []
    for _ in range(2):
        gW, gb, gbb = d.guarded(blocks, K, 32), d.guarded(1, blocks + 3, 32), d.guarded(blocks, K, 32)
        dZ16, dZ32 = d.guarded(B, ld16, 16), d.guarded(B, ld32, 32) if c.get("dz32", True) else None
        P = ctypes.c_int32(-1)
        d.ready()
        d.ffi.check(d.lib.orx_head16_bwd(d.ctx._h, d.ptr(X), h["ldx"], d.ptr(w), d.ptr(dy), d.ptr(pred), act, below, d.ptr(gW), d.ptr(gb),
                                         d.ptr(dZ16), ld16, d.ptr(dZ32), ld32, d.ptr(gbb), B, K, ctypes.byref(P)))
        d.ctx.synchronize()
        res.append(dict(gW=d.get(gW, np.uint32), gb=d.get(gb, np.uint32), gbb=d.get(gbb, np.uint32), dZ16=d.get(dZ16, np.uint16),
                        dZ32=d.get(dZ32, np.uint32) if dZ32 is not None else None, P=P.value))
    same_bits(res[0], res[1], what)
    r = res[0]
    P = r["P"]
    assert 1 <= P <= blocks, f"{what}: P = {P} of at most {blocks} blocks"
    want = ref.head_bwd(h["X"][:B, :K], h["w"][:K], h["dy"], h["pred"], act, below)
    check_guards(r["gW"], P, K, PAT32, what + " gW partial rows")
    check_guards(r["gbb"], P, K, PAT32, what + " gb_below partial rows")
    assert (r["gb"][0, P:] == PAT32).all() and (r["gb"][1:] == PAT32).all(), f"{what}: gb words beyond P were written"
    check_guards(r["dZ16"], B, K, PAT16, what + " dZ16")
    check_values(r["gW"][:P, :K].view(np.float32).astype(np.float64).sum(axis=0), want["gW"], None, what + " gW")
    check_values(r["gbb"][:P, :K].view(np.float32).astype(np.float64).sum(axis=0), want["gb_below"], None, what + " gb_below")
    check_values(np.float64(r["gb"][0, :P].view(np.float32).astype(np.float64).sum()).reshape(1), np.float64(want["gb"]).reshape(1), None, what + " gb")
    check_f16(r["dZ16"][:B, :K].view(np.float16), want["dZ"], None, what + " dZ16")
    if r["dZ32"] is not None:
        check_guards(r["dZ32"], B, K, PAT32, what + " dZ32")
        check_values(r["dZ32"][:B, :K].view(np.float32), want["dZ"], None, what + " dZ32")


def cast_source(M, N, seed=11):
    """fp32 values whose conversion is decided by the rounding rule: ties between neighbouring fp16 values (both parities), fp16
    subnormals and values below the smallest one, the overflow threshold 65520 (a tie that goes to inf) and its neighbours, +-0, inf"""
    rng = np.random.default_rng(seed)
    src = (rng.standard_normal((M, N)) * 2.0 ** rng.integers(-26, 17, (M, N))).astype(np.float32)
    h = rng.standard_normal((M, N)).astype(np.float16).astype(np.float32)
    ties = h + (np.spacing(np.abs(h).astype(np.float16)).astype(np.float32) / 2) * np.sign(h)      # exactly half way to the next fp16 value
    special = np.array([65504, 65519.996, 65520, 65536, -65520, 1e30, np.inf, -np.inf, 0.0, -0.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001,
                        3 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 5.96e-8, 1e-10], np.float32)
    pick = rng.uniform(size=(M, N))
    src = np.where(pick < 0.3, ties, src).astype(np.float32)
    flat = src.reshape(-1)
    flat[:min(special.size, flat.size)] = special[:flat.size]
    return src


def run_cast16(d, c):
    """cast16_kernel writes ALL ld16 columns of a row: the fp16 values below N, zeros from N on (the products read those
    columns as part of whole 16-byte chunks) -- so only rows beyond M are guards here"""
    M, N, lds, ld16 = c["M"], c["N"], c["lds"], c["ld16"]
    what = "cast16 " + c["id"]
    src = cast_source(M, N)
    sbuf = np.full((M + GUARD_ROWS, lds), np.nan, np.float32); sbuf[:M, :N] = src
    S = d.put(sbuf)
    res = []
    for _ in range(2):
        out = d.guarded(M, ld16, 16)
        d.ready()
        d.ffi.check(d.lib.orx_cast16(d.ctx._h, d.ptr(S), lds, d.ptr(out), ld16, M, N))
        d.ctx.synchronize()
        res.append(d.get(out, np.uint16))
    assert np.array_equal(res[0], res[1]), f"{what}: two runs differ"
    r = res[0]
    assert (r[M:] == PAT16).all(), f"{what}: rows beyond {M} were written"
    want = ref.cast16(src, ld16)
    assert np.array_equal(r[:M], want.view(np.uint16)), \
        f"{what}: {int((r[:M] != want.view(np.uint16)).sum())} halves differ from NumPy's round-to-nearest-even (columns >= N must be +0)"


def run_refusals(d, masks_ok=True):
    """shapes the kernels do not carry come back as ORX_ERR_ARG and nothing runs (return codes only)"""
    ERR = d.ffi.ORX_ERR_ARG
    rng = np.random.default_rng(0)
    A, B = d.put(operand16(rng, 128, 64, 64, "exact")), d.put(operand16(rng, 128, 64, 64, "exact"))
    nt_call(d, A, 60, B, 64, 128, 64, 60, "C", 68, 0, expect=ERR)                 # lda % 8 != 0
    nt_call(d, A, 64, B, 64, 128, 16, 64, "C", 68, 0, expect=ERR)                 # N < 32
    C0 = np.zeros((64, 64), np.float32)
    tn_call(d, A, 60, B, 64, C0, 68, None, 64, 64, 128, 1.0, expect=ERR)          # lda % 8 != 0
    tn_call(d, A, 64, B, 64, C0, 68, None, 64, 64, 128, 1.0, expect=ERR)          # one tile: split-K without a slab
    if not masks_ok:
        # a forced tile, register staging, the wave-tile experiment, ORX_GEMM16_NO_MASK: no relu masks
        C16 = d.guarded(128, 72, 16)
        m = d.guarded(1, 4096, 64)
        d.ready()
        rc = d.lib.orx_gemm16_nt(d.ctx._h, d.ptr(A), 64, d.ptr(B), 64, None, 0, d.ptr(C16), 72, None, 128, 64, 64, 1, None, None, 0, 0, None, None, d.ptr(m), None)
        assert rc == ERR, f"a relu mask with a form that has none: return code {rc}"
        d.ctx.synchronize()


RUNNERS = {"nt": run_nt, "tn": run_tn, "group": run_group, "head_fwd": run_head_fwd, "head_bwd": run_head_bwd, "cast16": run_cast16}


def case_form(kind, c, num_cu):
    """what the plan query says about a case row in THIS process (its environment)"""
    if kind == "nt":
        M, N, K, lda, ldb = nt_layout(c)
        return plan(num_cu, M, N, K, lda, ldb)[0]
    if kind == "tn":
        return plan(num_cu, c["M"], c["N"], c["K"], c.get("lda", up(c["M"], 128)), c.get("ldb", up(c["N"], 128)))[1]
    return group_plan(num_cu, c["B"], c["in"], c["out"], c["ldx"], c["lddz"], c["ldw"], c.get("nt_cols", 0))


def main():
    import test_gpu_gemm16 as T
    name = sys.argv[1]
    env, cases = T.ENV_SETS[name]
    for k, v in env.items():
        assert os.environ.get(k) == v, f"the parent did not set {k}={v}"
    if len(sys.argv) > 2 and sys.argv[2] == "--plan-only":          # no device: the forms this environment selects on 256 CUs
        for kind, c in cases:
            p = case_form(kind, c, 256)
            want = c.get("expect_form", {})
            assert {k: p[k] for k in want} == want, f"{kind} {c['id']}: written for {want}, the plan says {p}"
            print("PLAN", kind, c["id"], json.dumps(p), flush=True)
        print("DONE", len(cases), flush=True)
        return
    d = Dev()
    for kind, c in cases:
        p = RUNNERS[kind](d, c)
        want = c.get("expect_form")
        if want:
            got = {k: p[k] for k in want}
            assert got == want, f"{kind} {c['id']}: the case was written for {want}, this process runs {got}"
        print("CASE", kind, c["id"], "ok", flush=True)
    run_refusals(d, masks_ok=not any(k in env for k in ("ORX_GEMM16_TILE", "ORX_GEMM16_DMA", "ORX_GEMM16_WAVE_TILE", "ORX_GEMM16_NO_MASK")))
    print("DONE", len(cases), flush=True)


if __name__ == "__main__":
    main()
