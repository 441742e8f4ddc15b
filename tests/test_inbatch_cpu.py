"""CPU: the reference of the in-batch step (tests/inbatch_ref.py) against torch autograd in float64 on every shape, the masking of
the duplicate-heavy case, the launch geometry, the headroom of the per-row loss bound, and the declarations of the entry points."""
import os
import re

import numpy as np
import pytest

import inbatch_cases as ic
import inbatch_ref as ir
from conftest import ROOT


def _extras(case, step=0):
    """weights (some of them 0) and log-Q-like offsets of a case's step"""
    rng = np.random.default_rng(case["seed"] + 100 + step)
    w = rng.uniform(0, 2, case["B"]); w[::5] = 0.0
    off = rng.normal(0, 1, case["B"])
    return w, off


def _torch_objective(U, V, b, uid, pid, w, off, scale, mask_hits, l2_reg):
    """J by torch in float64 on the GATHERED rows (leaves), so that autograd returns per-occurrence gradients"""
    import torch
    t = lambda x: torch.tensor(np.asarray(x, np.float64))
    u = t(U[uid]).requires_grad_(); v = t(V[pid]).requires_grad_(); bj = t(b[pid, 0]).requires_grad_()
    s = scale * (u @ v.T + bj[None, :]) + t(off)[None, :]
    n = torch.tensor(ir.columns(pid, mask_hits))
    lse = torch.logsumexp(torch.where(n, s, torch.tensor(-np.inf, dtype=torch.float64)), 1)
    l = lse - torch.diagonal(s)
    loss = (t(w) * l).sum() / len(uid)
    l2 = 0.5 * ((u * u).sum() + (v * v).sum())
    (loss + l2_reg * l2).backward()
    return float(loss.detach()), float(l2.detach()), l.detach().numpy(), dict(gu=u.grad.numpy(), gv=v.grad.numpy(), gb=bj.grad.numpy())


@pytest.mark.parametrize("si", range(len(ic.SHAPES)))
@pytest.mark.parametrize("mask_hits", [True, False])
def test_reference_equals_torch_autograd_in_float64_on_every_shape(si, mask_hits):
    """weights (some 0), offsets, scale != 1, l2_reg != 1; the loss, the row losses and all three gradients"""
    B, D, NU, NI, chunk = ic.SHAPES[si]
    case = dict(opt="sgd", bias=True, K=1, mask=mask_hits, B=B, D=D, NU=NU, NI=NI, chunk=chunk, seed=300 + si)
    U, V, b, uid, pid = ic.make(case)
    U, V, b = (x.astype(np.float64) for x in (U, V, b))
    w, off = _extras(case)
    scale, l2_reg = 1.7, 0.3
    loss, l2 = ir.forward(U, V, b, uid[0], pid[0], w, off, scale, mask_hits)
    rows = ir.row_losses(U, V, b, uid[0], pid[0], off, scale, mask_hits)
    g = ir.grads(U, V, b, uid[0], pid[0], w, off, scale, mask_hits, l2_reg)
    tl, tl2, trows, tg = _torch_objective(U, V, b, uid[0], pid[0], w, off, scale, mask_hits, l2_reg)
    rtol = 1e-10
    assert abs(loss - tl) <= rtol * abs(tl) and abs(l2 - tl2) <= rtol * tl2
    assert np.abs(rows - trows).max() <= rtol * max(np.abs(trows).max(), 1e-300)
    for k in ("gu", "gv", "gb"):
        assert np.isfinite(g[k]).all()
        assert np.abs(g[k] - tg[k]).max() <= rtol * np.abs(tg[k]).max(), k
    if B == 1:
        assert rows[0] == 0.0 and np.array_equal(g["gu"], l2_reg * U[uid[0]]) and g["gb"][0] == 0.0


def test_the_duplicate_heavy_shape_exercises_the_masking():
    """at least a quarter of its rows have one or more masked columns; and the mask changes the loss"""
    B, D, NU, NI, chunk = ic.SHAPES[ic.DUP_SHAPE]
    found = 0
    for case in (c for c in ic.CASES if c["shape"] == ic.DUP_SHAPE):
        U, V, b, uid, pid = ic.make(case)
        for s in range(case["K"]):
            masked = (~ir.columns(pid[s], True)).sum(1)
            assert (masked >= 1).mean() >= 0.25, case["name"]
            on = ir.forward(U.astype(np.float64), V.astype(np.float64), None, uid[s], pid[s], mask_hits=True)[0]
            off = ir.forward(U.astype(np.float64), V.astype(np.float64), None, uid[s], pid[s], mask_hits=False)[0]
            assert abs(on - off) > 1e-3 * abs(off)
            found += 1
    assert found >= 4


def test_the_case_list_covers_the_shapes():
    assert len(ic.CASES) == 32
    for opt in ic.OPTS:
        mine = [c for c in ic.CASES if c["opt"] == opt]
        assert sorted(c["shape"] for c in mine) == list(range(len(ic.SHAPES)))
        assert {(c["bias"], c["K"], c["mask"]) for c in mine} == {(b, K, m) for b in (True, False) for K in (1, 3) for m in (True, False)}
    for si in range(len(ic.SHAPES)):
        assert len({(c["bias"], c["K"], c["mask"]) for c in ic.CASES if c["shape"] == si}) == len(ic.OPTS)


def test_the_geometry_of_the_launcher():
    from openrec_amd import runtime as rt
    for B, D, NU, NI, chunk in ic.SHAPES:
        g = rt.inbatch_geometry(B, D, chunk)
        assert g["dim"] == -(-D // 16) * 16 and g["dim"] >= D
        assert g["tile"] == 64, "the forced chunk widths of tests/inbatch_cases.py assume a tile of 64 columns"
        blocks = -(-B // g["rows"])
        if chunk:
            assert g["chunks"] == -(-B // chunk) and g["chunks"] > 1, (B, D)
        if B >= 130:
            assert blocks > 1, (B, D)
    assert rt.inbatch_geometry(130, 50, 64)["chunks"] == 3 and rt.inbatch_geometry(300, 128, 64)["chunks"] == 5
    assert rt.inbatch_geometry(1100, 16)["chunks"] > 1                  # the launcher's own chunking splits this one
    assert rt.inbatch_geometry(300, 128, 64) == rt.inbatch_geometry(300, 128, 64)
    for bad in (dict(chunk=-64), dict(chunk=48), dict(D=257), dict(D=0), dict(B=-1)):
        with pytest.raises(ValueError):
            rt.inbatch_geometry(**{**dict(B=300, D=64, chunk=0), **bad})


# ---- the per-row loss bound ---------------------------------------------------------------------------------------------------
def _rows_f32(s, n, order):
    """l_i in plain float32 from float32 scores s [B, B] and the column sets n, summing in `order`"""
    B = len(s)
    f = np.float32
    assert s.dtype == f
    sm = np.where(n, s, f(-np.inf))                                     # (a masked column adds exp(-inf) = 0: no rounding)
    tot = np.zeros(B, f)
    if order in ("forward", "reversed"):
        m = sm.max(1)
        e = np.exp(sm - m[:, None])
        for j in (range(B) if order == "forward" else range(B - 1, -1, -1)):
            tot = tot + e[:, j]
    else:                                                               # tiles of 64 columns, rescaled online
        m = np.full(B, -3.0e38, f)
        for j0 in range(0, B, 64):
            blk = sm[:, j0:j0 + 64]
            mn = np.maximum(m, blk.max(1))
            part = np.zeros(B, f)
            for j in range(blk.shape[1]):
                part = part + np.exp(blk[:, j] - mn)
            tot = tot * np.exp(m - mn) + part
            m = mn
    assert tot.dtype == f and m.dtype == f
    return (m + np.log(tot)) - np.diagonal(s)


@pytest.mark.parametrize("case", ic.CASES, ids=[c["name"] for c in ic.CASES])
def test_headroom_of_the_row_loss_bound_on_every_case(case):
    """The row losses in plain float32 NumPy -- forward, reversed, and in tiles of 64 with online rescaling -- stay within HALF the
    bound of inbatch_ref.row_bound against the float64 reference: the bound leaves room for a correct fp32 implementation."""
    U, V, b, uid, pid = ic.make(case)
    w, off = _extras(case)
    off32 = off.astype(np.float32)
    for scale in (1.0, 4.0):
        want = ir.row_losses(U.astype(np.float64), V.astype(np.float64), None if b is None else b.astype(np.float64), uid[0], pid[0],
                             off32.astype(np.float64), scale, case["mask"])
        bound = ir.row_bound(U, V, b, uid[0], pid[0], off32, scale, case["mask"])
        _, _, s = ir.scores(U, V, b, uid[0], pid[0], off32, np.float32(scale))
        assert s.dtype == np.float32
        n = ir.columns(pid[0], case["mask"])
        for order in ("forward", "reversed", "tiles"):
            got = _rows_f32(s, n, order)
            worst = (np.abs(got.astype(np.float64) - want) / bound).max()
            assert worst <= 0.5, (case["name"], scale, order, worst)


def test_the_bound_sees_a_dropped_column():
    """at B = 300 a dropped column moves lse by about 3e-3 against a bound of about 4e-5"""
    case = next(c for c in ic.CASES if c["B"] == 300)
    U, V, b, uid, pid = ic.make(case)
    U64, V64 = U.astype(np.float64), V.astype(np.float64)
    b64 = None if b is None else b.astype(np.float64)
    bound = ir.row_bound(U, V, b, uid[0], pid[0], None, 1.0, case["mask"])
    _, _, s = ir.scores(U64, V64, b64, uid[0], pid[0])
    n = ir.columns(pid[0], case["mask"])
    want = ir._lse(s, n)
    n2 = n.copy()
    drop = (np.arange(300) + 7) % 300
    n2[np.arange(300), drop] = False
    moved = np.abs(ir._lse(s, n2) - want)
    assert np.median(moved) > 10 * np.median(bound) and bound.max() < 2e-4


# ---- the boundary -------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_typed_and_exposed():
    hdr = open(os.path.join(ROOT, "include", "openrec_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    from openrec_amd import _ffi, runtime as rt
    for name, nargs in (("orx_inbatch_step", 18), ("orx_inbatch_loss", 15), ("orx_inbatch_geometry", 4)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert m, f"{name} is not declared in openrec_hip.h"
        assert len(m.group(1).split(",")) == nargs, name
        assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == nargs, name
    assert re.search(r"ORX_IB_MASK_HITS\s*=\s*0x1000", code) and _ffi.ORX_IB_MASK_HITS == 0x1000
    taken = (_ffi.ORX_IDS_DEVICE | _ffi.ORX_HOGWILD | _ffi.ORX_NO_L2 | _ffi.ORX_CENSOR | _ffi.ORX_POINT_SIGMOID | _ffi.ORX_OUT_DEVICE
             | _ffi.ORX_SHARD_OVERLAP | _ffi.ORX_SHARD_NO_DEDUP | _ffi.ORX_SHARD_DEDUP)
    assert _ffi.ORX_IB_MASK_HITS & taken == 0
    assert callable(rt.inbatch_step) and callable(rt.inbatch_loss) and callable(rt.inbatch_geometry)
    from openrec_amd.tf2.recommenders import BPR
    assert callable(BPR.train_steps_inbatch)


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
           dict(weights=np.ones(3, np.float32)), dict(item_offset=np.zeros(5, np.float32)), dict(l2_reg=-1.0), dict(l2_reg=float("nan")),
           dict(l2_reg=0.5, no_l2=True), dict(K=2, B=4), dict(B=4, id_stride=2), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")),
           dict(scale=float("nan")), dict(chunk=-64), dict(chunk=32)]
    for kw in bad:
        with pytest.raises(ValueError):
            rt.inbatch_step(**{**ok, **kw})
