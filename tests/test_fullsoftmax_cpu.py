"""CPU: the reference of the full-softmax step (tests/fullsoftmax_ref.py) against torch autograd in float64 on every shape, the
float32 reference against the float64 one under the yardsticks the GPU test uses (the per-row loss bound, conftest.delta_check,
TOL_ADAM), the launch geometry, and the declarations of the entry points."""
import os
import re

import numpy as np
import pytest

import fullsoftmax_cases as fc
import fullsoftmax_ref as fr
from conftest import ROOT, TOL_ADAM, delta_check, rel_err


def _extras(case):
    """weights (some of them 0) and a log-prior-like offset per ITEM"""
    rng = np.random.default_rng(case["seed"] + 100)
    w = rng.uniform(0, 2, case["B"]); w[::5] = 0.0
    off = rng.normal(0, 1, case["NI"])
    return w, off


def _f64(x):
    return None if x is None else x.astype(np.float64)


@pytest.mark.parametrize("si", range(len(fc.SHAPES)))
def test_reference_equals_torch_autograd_in_float64_on_every_shape(si):
    """weights (some 0), offsets, scale != 1, l2_reg != 0; the loss, the row losses, gu per occurrence and the DENSE gradients of
    the item table and the bias, the l2 term l2_reg n_j V[j] of the looked-up rows included"""
    import torch
    case = fc.shape_case(si, seed=300 + si)
    U, V, b, uid, pid = fc.make(case)
    U, V, b = _f64(U), _f64(V), _f64(b)
    w, off = _extras(case)
    scale, l2_reg = 1.7, 0.3
    t = lambda x: torch.tensor(np.asarray(x, np.float64))
    u = t(U[uid]).requires_grad_(); tv = t(V).requires_grad_(); tb = t(b[:, 0]).requires_grad_()
    s = scale * (u @ tv.T + tb[None, :]) + t(off)[None, :]
    lp = torch.tensor(pid.astype(np.int64))
    l = torch.logsumexp(s, 1) - s[torch.arange(len(pid)), lp]
    loss = (t(w) * l).sum() / len(pid)
    l2 = 0.5 * ((u * u).sum() + (tv[lp] * tv[lp]).sum())
    (loss + l2_reg * l2).backward()
    got = fr.forward(U, V, b, uid, pid, w, off, scale)
    rows = fr.row_losses(U, V, b, uid, pid, off, scale)
    g = fr.grads(U, V, b, uid, pid, w, off, scale, l2_reg)
    rtol = 1e-12
    assert abs(got[0] - loss.item()) <= rtol * abs(loss.item()) and abs(got[1] - l2.item()) <= rtol * l2.item()
    assert np.abs(rows - l.detach().numpy()).max() <= rtol * np.abs(rows).max()
    for k, want in (("gu", u.grad.numpy()), ("GV", tv.grad.numpy()), ("Gb", tb.grad.numpy())):
        assert g[k].shape == want.shape and np.isfinite(g[k]).all()
        assert np.abs(g[k] - want).max() <= rtol * np.abs(want).max(), k
    if fc.SHAPES[si][0] > fc.SHAPES[si][3]:                                   # more samples than items: labels repeat
        assert np.bincount(pid).max() > 1


def test_the_case_list_covers_the_shapes():
    assert len(fc.CASES) == 32
    for opt in fc.OPTS:
        mine = [c for c in fc.CASES if c["opt"] == opt]
        assert sorted(c["shape"] for c in mine) == list(range(len(fc.SHAPES)))
        assert {c["bias"] for c in mine} == {True, False}
    for si in range(len(fc.SHAPES)):
        assert {c["bias"] for c in fc.CASES if c["shape"] == si} == {True, False}


# ---- the float32 reference under the GPU test's yardsticks --------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.CASES, ids=[c["name"] for c in fc.CASES])
def test_the_float32_reference_stays_within_the_yardsticks(case):
    """The reference run in float32 against the reference run in float64: every row loss inside row_bound (the headroom is
    printed), every table after one step inside delta_check (SGD, Adagrad, momentum) or TOL_ADAM (Adam)."""
    U, V, b, uid, pid = fc.make(case)
    w, off = _extras(case)
    w32, off32 = w.astype(np.float32), off.astype(np.float32)
    for scale in (1.0, 4.0):
        want = fr.row_losses(_f64(U), _f64(V), _f64(b), uid, pid, _f64(off32), scale)
        got = fr.row_losses(U, V, b, uid, pid, off32, np.float32(scale))
        assert got.dtype == np.float32
        bound = fr.row_bound(U, V, b, uid, pid, off32, scale)
        worst = (np.abs(got.astype(np.float64) - want) / bound).max()
        print(f"{case['name']} scale {scale}: worst row at {worst:.3g} of the bound")
        assert worst <= 1.0, (case["name"], scale, worst)
    t32 = [U.copy(), V.copy(), None if b is None else b.copy()]
    t64 = [_f64(U), _f64(V), _f64(b)]
    fr.step(*t32, uid, pid, fc.make_opt(case["opt"]), w=w32, off=off32, scale=np.float32(1.0), l2_reg=np.float32(0.01))
    fr.step(*t64, uid, pid, fc.make_opt(case["opt"]), w=_f64(w32), off=_f64(off32), scale=1.0, l2_reg=float(np.float32(0.01)))
    for name, W0, got, want in zip(("user", "item", "bias"), (U, V, b), t32, t64):
        if W0 is None:
            continue
        assert got.dtype == np.float32
        if case["opt"] == "adam":
            assert rel_err(got, want.astype(np.float32)) <= TOL_ADAM, name
        else:
            delta_check(W0, got, want.astype(np.float32), steps=1, what=f"{case['name']} {name}")


def test_the_bound_sees_a_dropped_column_and_a_dropped_label_term():
    """A dropped column -- the label's own term is one -- moves lse_i by about pi_ij ~ 1 / NI, against a bound of about 2 NI u:
    one column is seen up to NI of a few hundred (checked at NI = 63 and 80), a dropped TILE of 64 columns at every shape
    (checked at NI = 5000, where a single column moves lse by 2e-4 against a bound of 6e-4)."""
    for si, ncols in ((1, 1), (6, 1), (5, 64)):
        case = fc.shape_case(si)
        U, V, b, uid, pid = fc.make(case)
        bound = fr.row_bound(U, V, b, uid, pid)
        s = fr.scores(_f64(U)[uid], _f64(V), _f64(b))
        want = fr._lse(s) - fr._label(s, pid)
        B, NI = s.shape
        s2 = s.copy()
        for k in range(ncols):
            s2[np.arange(B), (pid + 7 + k) % NI] = -np.inf                  # columns that are not the label
        moved = np.abs((fr._lse(s2) - fr._label(s, pid)) - want)
        assert np.median(moved) > 10 * np.median(bound) and bound.max() < 2e-3, (si, np.median(moved), np.median(bound))
        if ncols == 1:
            s3 = s.copy(); s3[np.arange(B), pid] = -np.inf                  # the label's own term missing from the sum
            moved = np.abs((fr._lse(s3) - fr._label(s, pid)) - want)
            assert np.median(moved) > 10 * np.median(bound), si


# ---- the geometry -------------------------------------------------------------------------------------------------------------
def test_the_geometry_of_the_launcher():
    from openrec_amd import runtime as rt
    for si, (B, D, NU, NI, ci, cs) in enumerate(fc.SHAPES):
        g = rt.fullsoftmax_geometry(B, NI, D, ci, cs)
        assert g["dim"] == -(-D // 16) * 16 and g["rows"] == 64
        assert g["tile"] == 64, "the forced chunk sizes of tests/fullsoftmax_cases.py assume a tile of 64"
        if si in fc.FORCED_CHUNKS:
            assert (g["item_chunks"], g["sample_chunks"]) == fc.FORCED_CHUNKS[si], (si, g)
        assert g["scratch_bytes"] > 0
        assert g == rt.fullsoftmax_geometry(B, NI, D, ci, cs)
    own = rt.fullsoftmax_geometry(1100, 2000, 16)
    assert own["item_chunks"] > 1 and own["sample_chunks"] > 1           # the launcher's own chunking splits both sides
    big = rt.fullsoftmax_geometry(4096, 1000000, 64)
    assert big["sample_chunks"] == 1 and big["scratch_bytes"] < 2 * 4096 * 1000000 * 4 // 8
    last = 0
    for B in (1, 64, 65, 1000, 4096, 20000):
        cur = rt.fullsoftmax_geometry(B, 5000, 64)["scratch_bytes"]
        assert cur >= last, B
        last = cur
    last = 0
    for NI in (1, 64, 65, 1000, 5000, 100000, 1000000):
        cur = rt.fullsoftmax_geometry(300, NI, 64)["scratch_bytes"]
        assert cur >= last, NI
        last = cur
    ok = dict(B=300, items=5000, D=64, chunk_items=0, chunk_samples=0)
    for bad in (dict(chunk_items=-64), dict(chunk_items=48), dict(chunk_samples=-64), dict(chunk_samples=100), dict(D=257), dict(D=0),
                dict(B=-1), dict(B=2 ** 31), dict(items=2 ** 31), dict(items=0)):
        with pytest.raises(ValueError):
            rt.fullsoftmax_geometry(**{**ok, **bad})


# ---- the boundary -------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_typed_and_exposed():
    hdr = open(os.path.join(ROOT, "include", "openrec_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    from openrec_amd import _ffi, runtime as rt
    for name, nargs in (("orx_fullsoftmax_step", 18), ("orx_fullsoftmax_loss", 15), ("orx_fullsoftmax_geometry", 6),
                        ("orx_seqrec_full_step", 22), ("orx_seqrec_full_loss", 19)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert m, f"{name} is not declared in openrec_hip.h"
        assert len(m.group(1).split(",")) == nargs, name
        assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == nargs, name
        assert hasattr(_ffi.load(), name), name
    assert callable(rt.fullsoftmax_step) and callable(rt.fullsoftmax_loss) and callable(rt.fullsoftmax_geometry)
    assert callable(rt.SeqRec.step_full) and callable(rt.SeqRec.loss_full)
    from openrec_amd.tf2.recommenders import BPR, VanillaYouTubeRec
    assert callable(BPR.train_steps_full) and callable(VanillaYouTubeRec.train_steps_full) and callable(VanillaYouTubeRec.loss_full)


def test_bad_arguments_are_value_errors_before_the_library_is_called():
    """(no table handle is ever dereferenced: the stand-ins have only a shape)"""
    from openrec_amd import runtime as rt

    class T:
        def __init__(self, r, d):
            self.shape = (r, d)
    U, V, b = T(10, 8), T(12, 8), T(12, 1)
    ids = np.zeros(4, np.int32)
    ok = dict(opt=None, user=U, item=V, bias=b, uid=ids, pid=ids)
    bad = [dict(user=T(10, 4)), dict(user=T(10, 260), item=T(12, 260)), dict(bias=T(11, 1)), dict(bias=T(12, 2)), dict(pid=np.zeros(3, np.int32)),
           dict(weights=np.ones(3, np.float32)), dict(item_offset=np.zeros(4, np.float32)), dict(item_offset=np.zeros(13, np.float32)),
           dict(l2_reg=-1.0), dict(l2_reg=float("nan")), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan")),
           dict(chunk_items=-64), dict(chunk_items=32), dict(chunk_samples=-64), dict(chunk_samples=100), dict(train=("users",)), dict(train=()),
           dict(train=("bias",), bias=None)]
    for kw in bad:
        with pytest.raises(ValueError):
            rt.fullsoftmax_step(**{**ok, **kw})
    for kw in (dict(scale=0.0), dict(chunk_items=32), dict(item_offset=np.zeros(4, np.float32)), dict(pid=np.zeros(3, np.int32))):
        with pytest.raises(ValueError):
            rt.fullsoftmax_loss(**{**{k: v for k, v in ok.items() if k != "opt"}, **kw})
