"""CPU: the reference of the tower step (tests/tower_ref.py) against torch autograd in float64 on every case, the float32
restatement against the float64 one under the yardsticks the GPU test uses (conftest.delta_check, TOL, TOL_ADAM), the launch
geometry, the declarations of the entry points and the runtime's refusals."""
import os
import re

import numpy as np
import pytest

import fullsoftmax_ref as fr
import runtime_standin as rs
import tower_cases as tc
import tower_ref as tr
from conftest import ROOT, TOL, TOL_ADAM, delta_check, rel_err

_MODELS = {}


def _model(case):
    key = case["name"]
    if key not in _MODELS:
        _MODELS[key] = tc.make(case)          # (the seed search runs once per case; nobody writes into the cached model)
    return _MODELS[key]


def _extras(case):
    rng = np.random.default_rng(case["seed"] + 100)
    w = rng.uniform(0, 2, case["B"]).astype(np.float32); w[::5] = 0.0
    return w, rng.normal(0, 1, case["NI"]).astype(np.float32)


def _tables(m):
    out = [("history", m["H"]), ("item", m["V"]), ("bias", m["b"])]
    out += [(f"side{j}", s) for j, s in enumerate(m["S"])]
    for l, (W, c) in enumerate(m["layers"]):
        out += [(f"W{l}", W), (f"c{l}", c)]
    return [(k, v) for k, v in out if v is not None]


@pytest.mark.parametrize("si", range(len(tc.SHAPES)))
def test_reference_equals_torch_autograd_in_float64(si):
    """weights (some 0), offsets, scale != 1, both l2 coefficients != 0: the losses and the gradient of every table"""
    import torch
    case = tc.shape_case(si)
    m = tc.copy_model(_model(case), np.float64)
    w, off = (x.astype(np.float64) for x in _extras(case))
    scale, l2_reg, l2_mlp = 1.7, 0.3, 0.2
    t = lambda x: torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    H, V = t(m["H"]), t(m["V"])
    b = t(m["b"][:, 0]) if m["b"] is not None else None
    S = [t(s) for s in m["S"]]
    layers = [(t(W), t(c[0]) if c is not None else None) for W, c in m["layers"]]
    ptr, items, pid = m["ptr"], m["items"], torch.tensor(m["pid"].astype(np.int64))
    B = case["B"]
    pooled = []
    for i in range(B):
        lo, hi = int(ptr[i]), int(ptr[i + 1])
        pooled.append(H[torch.tensor(items[lo:hi].astype(np.int64))].mean(0) if hi > lo else torch.zeros(case["Dh"], dtype=torch.float64))
    x0 = torch.cat([s[torch.tensor(f.astype(np.int64))] for s, f in zip(S, m["f"])] + [torch.stack(pooled)], 1)
    x = x0
    for l, (W, c) in enumerate(layers):
        x = x @ W if c is None else x @ W + c[None, :]
        if l + 1 < len(layers) or case["relu_last"]:
            x = torch.relu(x)
    s = x @ V.T
    if b is not None:
        s = s + b[None, :]
    s = scale * s + torch.tensor(off)[None, :]
    rows = torch.logsumexp(s, 1) - s[torch.arange(B), pid]
    loss = (torch.tensor(w) * rows).sum() / B
    l2 = 0.5 * ((x0 * x0).sum() + (V[pid] * V[pid]).sum())
    reg = sum((W * W).sum() + ((c * c).sum() if c is not None else 0.0) for W, c in layers)
    (loss + l2_reg * l2 + l2_mlp * 0.5 * reg).backward()

    args = (m["H"], m["V"], m["b"], m["S"], m["layers"], ptr, items, m["f"], m["pid"], "mean", case["relu_last"])
    got = tr.forward(*args, w, off, scale)
    g = tr.grads(*args, w, off, scale, l2_reg, l2_mlp)
    rtol = 1e-12
    assert abs(got[0] - loss.item()) <= rtol * abs(loss.item()) and abs(got[1] - l2.item()) <= rtol * l2.item()
    assert np.abs(tr.row_losses(*args, off, scale) - rows.detach().numpy()).max() <= rtol * rows.abs().max().item()

    def same(name, mine, want):
        assert mine.shape == want.shape and np.isfinite(mine).all(), name
        assert np.abs(mine - want).max() <= rtol * max(np.abs(want).max(), 1e-300), name
    same("GV", g["GV"], V.grad.numpy())
    if b is not None:
        same("Gb", g["Gb"], b.grad.numpy())
    for l, (W, c) in enumerate(layers):
        same(f"dW{l}", g["dW"][l], W.grad.numpy())
        if c is not None:
            same(f"dc{l}", g["dc"][l][0], c.grad.numpy())
    GH = np.zeros_like(m["H"]); np.add.at(GH, items, g["gh"])
    same("GH", GH, H.grad.numpy() if H.grad is not None else np.zeros_like(GH))
    for j, s in enumerate(S):
        GS = np.zeros_like(m["S"][j]); np.add.at(GS, m["f"][j], g["gS"][j])
        same(f"GS{j}", GS, s.grad.numpy())


def test_the_case_list_covers_the_shapes_and_the_margin_holds():
    assert len(tc.CASES) == 4 * len(tc.SHAPES)
    for opt in tc.OPTS:
        assert sorted(c["shape"] for c in tc.CASES if c["opt"] == opt) == list(range(len(tc.SHAPES)))
    assert {c["B"] for c in tc.CASES} == {1, 64, 65, 130} and {c["NI"] for c in tc.CASES} == {40, 300}
    assert {len(c["outs"]) for c in tc.CASES} == {1, 2, 3} and {len(c["side"]) for c in tc.CASES} == {0, 2}
    for si in range(len(tc.SHAPES)):
        case = tc.shape_case(si)
        m = _model(case)
        assert tc.margin_ok(m, case["relu_last"])
    # the exact zeros of the widest case are there: bag 0 is empty, no side row, no bias
    m = _model(tc.shape_case(1))
    x0, _, _ = tr.input_rows(m["H"], m["S"], m["ptr"], m["items"], m["f"], "mean")
    assert m["ptr"][1] == 0 and not tr.tower(x0, m["layers"])[1][0][0].any()
    # and a margin that is broken is seen
    m2 = tc.copy_model(m)
    m2["layers"][0][0][:, 3] = 0.0; m2["layers"][0][0][0, 3] = 1e-7; m2["layers"][0][0][1, 3] = -1e-7
    m2["H"][:, :2] = 0.25
    assert not tc.margin_ok(m2, True)


def _shrunk(case):
    """The wide-in shape at B = 12 for the float32 restatement.  At B = 130 each row of its 2-row side table has 65 occurrences, and
    the oracle's sparse SGD / momentum rules subtract them from the row one by one in float32: 65 roundings of a 0.2-sized
    element against delta_check's two -- measured 1.57 x the bound on side0 under SGD, while the summed gradient itself is within
    2e-7 of the float64 one (0.06 x the bound).  That is the oracle's order of subtraction, not the formulas: the device sums a
    row's occurrences first, and tests/test_gpu_tower.py keeps B = 130 against the float64 reference.  The same under SGD for the
    widest shape's history table (65 bags over 40 items, about six occurrences per row, 10 240 elements: the worst at 1.5 x the
    bound): B = 9 there.  Shrunk, the worst table element of either sits at 0.5 x its bound."""
    if case["shape"] == 0:
        return dict(case, B=12, name=case["name"] + "-B12")
    if case["shape"] == 1 and case["opt"] == "sgd":
        return dict(case, B=9, name=case["name"] + "-B9")
    return case


@pytest.mark.parametrize("case", tc.CASES, ids=[c["name"] for c in tc.CASES])
def test_the_float32_reference_stays_within_the_yardsticks(case):
    """The reference run in float32 against the reference run in float64, one step: every row loss inside
    fullsoftmax_ref.row_bound_q evaluated on the float64 queries, loss and l2 inside TOL, every table inside delta_check (SGD,
    Adagrad, momentum) or TOL_ADAM (Adam).  The worst ratio to the bound is printed per table."""
    case = _shrunk(case)
    m = _model(case)
    w, off = _extras(case)
    a32, a64 = tc.copy_model(m), tc.copy_model(m, np.float64)
    lists = lambda a: (a["H"], a["V"], a["b"], a["S"], a["layers"], m["ptr"], m["items"], m["f"], m["pid"])
    q64 = tr.queries(a64["H"], a64["S"], a64["layers"], m["ptr"], m["items"], m["f"], "mean", case["relu_last"])
    want_rows = fr.row_losses_q(q64, a64["V"], a64["b"], m["pid"], tc.f64(off))
    got_rows = tr.row_losses(*lists(a32), "mean", case["relu_last"], off)
    bound = fr.row_bound_q(q64, a64["V"], a64["b"], m["pid"], off)
    print(f"{case['name']}: worst row at {(np.abs(got_rows - want_rows) / bound).max():.3g} of the bound")
    assert (np.abs(got_rows - want_rows) <= bound).all()
    l32 = tr.step(*lists(a32), tc.make_opt(case["opt"]), "mean", case["relu_last"], w, off, np.float32(1.0), np.float32(0.01), np.float32(0.02))
    l64 = tr.step(*lists(a64), tc.make_opt(case["opt"]), "mean", case["relu_last"], tc.f64(w), tc.f64(off), 1.0,
                  float(np.float32(0.01)), float(np.float32(0.02)))
    assert abs(l32[0] - l64[0]) <= TOL * abs(l64[0]) and abs(l32[1] - l64[1]) <= TOL * abs(l64[1])
    for (name, W0), (_, got), (_, want) in zip(_tables(m), _tables(a32), _tables(a64)):
        assert got.dtype == np.float32
        w32 = want.astype(np.float32)
        print(f"{case['name']} {name}: rel err {rel_err(got, w32):.3g} ({rel_err(got, w32) / (TOL_ADAM if case['opt'] == 'adam' else TOL):.3g} of the table bound)")
        if case["opt"] == "adam":
            assert rel_err(got, w32) <= TOL_ADAM, name
        else:
            delta_check(W0, got, w32, steps=1, what=f"{case['name']} {name}")
            d = got.astype(np.float64) - w32
            ulp = np.spacing(np.maximum(np.maximum(np.abs(w32), np.abs(W0)), np.float32(np.abs(w32.astype(np.float64) - W0).max()))).astype(np.float64)
            print(f"{case['name']} {name}: worst element at {(np.abs(d) / (1e-5 * np.abs(w32.astype(np.float64) - W0) + 2 * ulp)).max():.3g} of the update bound")


# ---- the geometry, the boundary ----------------------------------------------------------------------------------------------
def test_the_geometry_of_the_launcher():
    from openrec_amd import runtime as rt
    g = rt.tower_geometry(130, (58, 70, 50))
    assert g["tile"] == 64 and g["batch_chunks"] == 3 and g["tiles_per_chunk"] == 1 and g["scratch_bytes"] > 0
    big = rt.tower_geometry(65536, (80, 256, 128, 64))
    assert big["batch_chunks"] == 32 and big["tiles_per_chunk"] == 32
    assert big["scratch_bytes"] < 16 * 65536 * (80 + 256 + 128 + 64) + 40 * 4 * (80 * 256 + 256 * 128 + 128 * 64 + 448)      # O(B sum of widths) and the partials
    last = 0
    for B in (1, 64, 65, 1000, 4096, 20000):
        cur = rt.tower_geometry(B, (58, 70, 50))["scratch_bytes"]
        assert cur >= last
        last = cur
    for bad in ((58,), (58, 70, 50, 40, 30, 20), (58, 0), (257, 10), (58, 300)):
        with pytest.raises(ValueError):
            rt.tower_geometry(64, bad)


def test_the_entry_points_are_declared_typed_and_exposed():
    hdr = open(os.path.join(ROOT, "include", "openrec_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    from openrec_amd import _ffi, runtime as rt
    for name, nargs in (("orx_tower_step", 30), ("orx_tower_loss", 26), ("orx_tower_query", 18), ("orx_tower_geometry", 4)):
        mm = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert mm, f"{name} is not declared in openrec_hip.h"
        assert len(mm.group(1).split(",")) == nargs, name
        assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == nargs, name
        assert hasattr(_ffi.load(), name), name
    assert (_ffi.ORX_TRAIN_SIDE, _ffi.ORX_TRAIN_TOWER) == (16, 32)
    assert re.search(r"ORX_TRAIN_SIDE\s*=\s*16\s*,\s*ORX_TRAIN_TOWER\s*=\s*32", code)
    for name in ("step_full", "loss_full", "user_table", "recommend"):
        assert callable(getattr(rt.DeepSeqRec, name))
    from openrec_amd.tf2.recommenders import VanillaYouTubeRec, YouTubeRec
    assert callable(YouTubeRec.train_steps_full) and callable(YouTubeRec.loss_full) and callable(VanillaYouTubeRec.train_steps_full)


def test_bad_arguments_are_value_errors_before_the_library_is_called():
    """on tests/runtime_standin.py's tables: handles only, and a library that records -- nothing may reach it"""
    from openrec_amd import runtime as rt
    ctx = rs.RecordingContext()
    T = lambda name, r, d, c=ctx: rs.StandinTable(c, name, r, d)
    H, V, b = T("H", 30, 8), T("V", 30, 6), T("b", 30, 1)
    S = [T("S0", 2, 3), T("S1", 9, 5)]
    W0, c0, W1, c1 = T("W0", 16, 10), T("c0", 1, 10), T("W1", 10, 6), T("c1", 1, 6)
    ok = dict(H=H, V=V, b=b, layers=[(W0, c0), (W1, c1)], side=S)
    bad = [dict(layers=[]), dict(layers=[(W0, c0)] * 5), dict(side=S * 3), dict(layers=[(W0, c0), (T("W", 11, 6), None)]),
           dict(layers=[(W0, c0), (W1, T("c", 6, 1))]), dict(layers=[(W0, c0), (T("W", 10, 7), None)]), dict(layers=[(W0, c0), (W1, c0)]),
           dict(V=H), dict(side=[S[0], S[0]]), dict(b=T("b", 29, 1)), dict(V=T("V", 31, 6)), dict(H=T("H", 30, 8, rs.RecordingContext())),
           dict(side=[], layers=[(T("W", 8, 300), None), (T("W", 300, 6), None)]), dict(pool="median"), dict(layers=[(None, c0)])]
    for kw in bad:
        with pytest.raises(ValueError):
            rt.DeepSeqRec(**{**ok, **kw})
    net = rt.DeepSeqRec(**ok)
    assert net.widths == [16, 10, 6]
    ptr, items = np.arange(0, 10, 2, dtype=np.int32), np.ones(8, np.int32)
    ids = np.zeros(4, np.int32)
    good = dict(opt=rs.StandinOptimizer(), bags=(ptr, items), pid=ids, side_ids=(ids, ids))
    bad = [dict(side_ids=(ids,)), dict(side_ids=(ids, np.zeros(3, np.int32))), dict(pid=np.zeros(5, np.int32)), dict(l2_mlp=-1.0),
           dict(l2_mlp=float("nan")), dict(l2_reg=-1.0), dict(scale=0.0), dict(chunk_items=32), dict(chunk_samples=-64), dict(train=("layers",)),
           dict(train=()), dict(weights=np.ones(3, np.float32)), dict(item_offset=np.zeros(4, np.float32)),
           dict(side_ids=(ids, rs.FakeDeviceTensor(4))), dict(bags=(ptr[::-1].copy(), items))]
    for kw in bad:
        with pytest.raises(ValueError):
            net.step_full(**{**good, **kw})
    with pytest.raises(ValueError):
        rt.DeepSeqRec(H, V, None, [(W0, c0), (W1, c1)], S).step_full(**{**good, "train": ("bias",)})
    with pytest.raises(ValueError):
        rt.DeepSeqRec(T("H", 30, 16), V, b, [(W0, c0), (W1, c1)]).step_full(**{**good, "side_ids": (), "train": ("side",)})
    for kw in (dict(side_ids=(ids,)), dict(scale=-1.0), dict(pid=np.zeros(3, np.int32))):
        with pytest.raises(ValueError):
            net.loss_full(**{**{k: v for k, v in good.items() if k != "opt"}, **kw})
    with pytest.raises(ValueError):
        net.user_table((ptr, items), (ids,))
    with pytest.raises(ValueError):
        net.user_table((ptr, items), (ids, ids), out=T("Q", 4, 7))
    assert not ctx._lib.calls
