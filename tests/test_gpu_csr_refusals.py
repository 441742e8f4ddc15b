"""GPU: what the library itself refuses of a malformed HOST CSR in the calls that walk a row range of a CSR against a table --
orx_als_half_step, orx_als_half_step_cg, orx_graph_spmm, orx_als_objective -- through the raw C ABI (`ALSCsr` refuses such input in
Python first).  Every refusal is ORX_ERR_ARG and leaves every table's bits alone; the context then computes what a fresh one does."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NR, NC, D = 6, 5, 8
PTR = np.array([0, 2, 3, 3, 6, 8, 9], np.int64)            # row 2 is empty
COLS = np.array([0, 3, 1, 0, 2, 4, 1, 3, 2], np.int32)
A, B, REG, CG_STEPS = 2.0, 1.0, 0.1, 3


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _tables(rt, ctx):
    rng = np.random.default_rng(7)
    small = rng.uniform(-0.5, 0.5, (NC, D)).astype(np.float32)       # the fixed table / the propagated table / the item table
    large = rng.uniform(-0.5, 0.5, (NR, D)).astype(np.float32)       # the solved table / the output / the user table
    return rt.Table(NC, D, ctx).write(small), rt.Table(NR, D, ctx).write(large), small, large


def _calls(lib, ctx, T, X):
    """the three row-range calls as f(row_ptr, cols, row0, nrows) -> code; row_ptr and cols are arrays or None"""
    def ptr(a):
        return a.ctypes.data if a is not None else None
    return {
        "orx_als_half_step": lambda rp, cols, row0=0, nrows=NR:
            lib.orx_als_half_step(ctx._h, T._h, X._h, ptr(rp), ptr(cols), None, row0, nrows, A, B, REG, 0),
        "orx_als_half_step_cg": lambda rp, cols, row0=0, nrows=NR:
            lib.orx_als_half_step_cg(ctx._h, T._h, X._h, ptr(rp), ptr(cols), None, row0, nrows, A, B, REG, CG_STEPS, 0),
        "orx_graph_spmm": lambda rp, cols, row0=0, nrows=NR:
            lib.orx_graph_spmm(ctx._h, T._h, X._h, None, 0.0, ptr(rp), ptr(cols), None, None, row0, nrows, -1, 0),
    }


def test_malformed_host_csr_is_refused_by_the_library():
    from openrec_amd import _ffi
    from openrec_amd import runtime as rt
    lib = _ffi.load()
    ctx, fresh = rt.default_context(), rt.Context(0)
    decreasing = PTR.copy(); decreasing[2] = 1             # row 1 ends before it starts
    negative = PTR.copy(); negative[0] = -1
    for name in ("orx_als_half_step", "orx_als_half_step_cg", "orx_graph_spmm"):
        T, X, small, large = _tables(rt, ctx)
        call = _calls(lib, ctx, T, X)[name]
        for what, rp, cols in (("decreasing", decreasing, COLS), ("negative first offset", negative, COLS), ("NULL row_ptr", None, COLS),
                               ("NULL cols", PTR, None)):
            assert call(rp, cols) == _ffi.ORX_ERR_ARG, (name, what)
        assert call(decreasing, COLS, 1, 2) == _ffi.ORX_ERR_ARG, name      # ... inside a range that does not start at row 0
        ctx.synchronize()
        assert np.array_equal(_bits(T.read()), _bits(small)) and np.array_equal(_bits(X.read()), _bits(large)), name
        # NULL cols with no entry in the range is accepted: the empty row 2 becomes zero, no other row is touched
        assert call(PTR, None, 2, 1) == _ffi.ORX_OK, name
        want = large.copy(); want[2] = 0.0
        assert np.array_equal(_bits(X.read()), _bits(want)) and np.array_equal(_bits(T.read()), _bits(small)), name
        # a valid call afterwards: the bits of a context that never saw a refusal
        Tf, Xf, _, _ = _tables(rt, fresh)
        assert call(PTR, COLS) == _ffi.ORX_OK and _calls(lib, fresh, Tf, Xf)[name](PTR, COLS) == _ffi.ORX_OK, name
        got = X.read()
        assert np.isfinite(got).all() and not np.array_equal(_bits(got), _bits(want)), name
        assert np.array_equal(_bits(got), _bits(Xf.read())) and np.array_equal(_bits(T.read()), _bits(small)), name

    # orx_als_objective takes the whole CSR: its own rules
    V, U, small, large = _tables(rt, ctx)
    Vf, Uf, _, _ = _tables(rt, fresh)
    out = ctypes.c_double(-1.0)

    def objective(c, user, item, rp, host_out):
        return lib.orx_als_objective(c._h, user._h, item._h, rp.ctypes.data, COLS.ctypes.data, None, A, B, REG, 0, host_out)

    shifted = PTR + 1                                      # row_ptr[0] != 0
    assert objective(ctx, U, V, shifted, ctypes.byref(out)) == _ffi.ORX_ERR_ARG
    assert objective(ctx, U, V, decreasing, ctypes.byref(out)) == _ffi.ORX_ERR_ARG
    assert objective(ctx, U, V, PTR, None) == _ffi.ORX_ERR_ARG
    ctx.synchronize()
    assert out.value == -1.0
    assert np.array_equal(_bits(U.read()), _bits(large)) and np.array_equal(_bits(V.read()), _bits(small))
    ref = ctypes.c_double(-1.0)
    assert objective(ctx, U, V, PTR, ctypes.byref(out)) == _ffi.ORX_OK and objective(fresh, Uf, Vf, PTR, ctypes.byref(ref)) == _ffi.ORX_OK
    assert np.isfinite(out.value) and out.value > 0.0 and out.value == ref.value
    assert np.array_equal(_bits(U.read()), _bits(large)) and np.array_equal(_bits(V.read()), _bits(small))
