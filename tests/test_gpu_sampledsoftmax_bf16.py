"""GPU: the sampled softmax over a shared candidate list with bf16 operands on the matrix cores (precision="bf16", ORX_SS_BF16)
against the rounded semantics of include/openrec_hip.h in float64: sampledsoftmax_ref on bf(Q), bf(V), bf(x) a torch.bfloat16
round trip.

Row losses are held to sampledsoftmax_ref.row_bound on the rounded tables: products of bf16 values are exact in fp32 and the
instruction sums them in fp32, so the fp32 path's bound holds as it stands; the loss and l2 bounds are the fp32 test's, l2 against
the unrounded rows.  An element of an SGD update: rel = 2^-8 + 2 row_bound + (max(B, S) + 8) u on a row's coefficients -- 2^-9 is
the coefficient's bf16 rounding, doubled for the device's own a; the rest is the fp32 test's -- and without the 2^-8 on the bias,
which sums unrounded coefficients; plus the fp32 test's ulp and occurrence terms."""
import numpy as np
import pytest
import torch

import fullsoftmax_cases as fc
import sampledsoftmax_ref as sr
from test_gpu_sampledsoftmax import LR, NI, NU, make

pytestmark = pytest.mark.gpu

U32 = sr.U32
# (B, S, D): k-padding below and between multiples of 32, tile edges on both axes; S = 520: three candidate chunks, the last of one
# tile; B = 300: two sample chunks
SHAPES = ((1, 1, 8), (63, 65, 20), (65, 63, 40), (65, 200, 64), (130, 65, 256), (3, 520, 64), (130, 520, 32), (300, 65, 64))
ids = lambda s: "B%d-S%d-D%d" % s


def _rt():
    from openrec_amd import runtime as rt
    return rt


def bf(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).bfloat16().float().numpy()


def _tables(rt, k):
    return tuple(None if x is None else rt.Table(*x.shape).write(x) for x in (k["U"], k["V"], k["b"]))


def _kw(k, **more):
    return dict(weights=k["w"], cand_offset=k["coff"], pos_offset=k["poff"], precision="bf16", **more)


def _ref(k, mask_hits=True, scale=1.0):
    """the reference's arguments on the rounded tables"""
    return (bf(k["U"])[k["uid"]], bf(k["V"]), k["b"], k["pid"], k["cand"]), dict(cand_off=k["coff"], pos_off=k["poff"], scale=scale, mask_hits=mask_hits)


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def test_the_shapes_cross_a_candidate_chunk_and_a_sample_chunk():
    rt = _rt()
    assert rt.sampled_softmax_geometry(3, 520, 64, precision="bf16")["cand_chunks"] == 3
    assert rt.sampled_softmax_geometry(300, 65, 64, precision="bf16")["sample_chunks"] == 2
    assert rt.sampled_softmax_geometry(130, 65, 40, precision="bf16")["dim"] == 64


# ---- 1. row losses, loss, l2 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_hits", [True, False])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_row_losses_loss_and_l2(shape, mask_hits):
    rt, k = _rt(), make(*shape)
    B, S, D = shape
    for scale in (1.0, 4.0):
        loss, l2, rows = rt.sampled_softmax_loss(*_tables(rt, k), k["uid"], k["pid"], k["cand"], **_kw(k, scale=scale, mask_hits=mask_hits, per_row=True))
        a, kw = _ref(k, mask_hits, scale)
        want, bound = sr.row_losses(*a, **kw), sr.row_bound(*a, **kw)
        wl = sr.forward(*a, w=k["w"], **kw)[0]
        wl2 = sr.forward(k["U"][k["uid"]], k["V"], k["b"], k["pid"], k["cand"], w=k["w"], **kw)[1]      # the unrounded rows
        err = np.abs(rows - want)
        print(f"{shape} mask={mask_hits} scale={scale}: worst row {(err / bound).max():.3g} x bound")
        assert rows.shape == (B,) and (err <= bound).all(), float((err / bound).max())
        c = k["w"].astype(np.float64) / B
        assert abs(loss - wl) <= (c * bound).sum() + (B + 8) * U32 * (c * np.abs(want)).sum() + U32 * abs(wl)
        assert abs(l2 - wl2) <= (D + B + 16) * U32 * wl2


# ---- 2. the rounding is where the semantics put it -----------------------------------------------------------------------------------
def test_the_rows_are_those_of_the_rounded_tables_and_not_of_the_fp32_tables():
    """(65, 63, 40): on the CPU the two float64 references differ by more than the sum of both bounds on 0.91 of the rows"""
    rt, k = _rt(), make(65, 63, 40)
    rows = rt.sampled_softmax_loss(*_tables(rt, k), k["uid"], k["pid"], k["cand"], **_kw(k, per_row=True))[2].astype(np.float64)
    a, kw = _ref(k)
    exact = (k["U"][k["uid"]], k["V"]) + a[2:]
    inside = np.abs(rows - sr.row_losses(*a, **kw)) <= sr.row_bound(*a, **kw)
    outside = np.abs(rows - sr.row_losses(*exact, **kw)) > sr.row_bound(*exact, **kw)
    print(f"{outside.mean():.2f} of the rows outside the bound of the unrounded tables")
    assert inside.all() and outside.mean() > 0.5


# ---- 3. one SGD step element by element ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shape", [(1, 1, 8), (65, 63, 40), (130, 65, 256), (3, 520, 64), (300, 65, 64)], ids=ids)
def test_one_sgd_step_element_by_element(shape, bias):
    rt, k = _rt(), make(*shape, bias=bias)
    B, S, D = shape
    tabs, l2_reg = _tables(rt, k), float(np.float32(0.01))
    rt.sampled_softmax_step(rt.Optimizer.sgd(LR), *tabs, k["uid"], k["pid"], k["cand"], **_kw(k, scale=2.0, l2_reg=l2_reg))
    a, kw = _ref(k, scale=2.0)
    rel = 2 * sr.row_bound(*a, **kw) + (max(B, S) + 8) * U32
    g, gb = sr.grads(*a, w=k["w"], rel=2.0 ** -8 + rel, **kw), sr.grads(*a, w=k["w"], rel=rel, **kw)
    lq, lv = l2_reg * k["U"][k["uid"]].astype(np.float64), np.zeros((B + S, D))       # the l2 terms, from the unrounded rows
    lv[:B] = l2_reg * k["V"][k["pid"]]
    checks = [("user", k["U"], tabs[0], k["uid"], g["gq"] + lq, g["tq"] + 2 * U32 * np.abs(lq)),
              ("item", k["V"], tabs[1], g["rows"], g["gV"] + lv, g["tV"] + 2 * U32 * np.abs(lv))]
    if bias:
        checks.append(("bias", k["b"], tabs[2], g["rows"], g["gb"][:, None], gb["tb"][:, None]))
    for name, W0, t, rows, grad, tol in checks:
        got, n = t.read().astype(np.float64), len(W0)
        delta, want = got - W0, -LR * sr.scatter(n, rows, grad)
        cnt = sr.scatter(n, rows, np.ones((len(rows), 1)))
        allowed = LR * sr.scatter(n, rows, tol) + (cnt + 2) * U32 * np.abs(want) + 2 * U32 * np.abs(W0)
        print(f"{shape} {name}: worst element {(np.abs(delta - want) / np.maximum(allowed, 1e-300)).max():.3g} x bound")
        assert (np.abs(delta - want) <= allowed).all(), name
        assert np.array_equal(_bits(t.read())[cnt[:, 0] == 0], _bits(W0)[cnt[:, 0] == 0]), f"{name}: an untouched row changed"
        assert np.abs(delta).max() > 0 or np.abs(want).max() < 1e-9      # (S = 1 with its one candidate masked: no bias gradient)


# ---- 4. consistency ------------------------------------------------------------------------------------------------------------------
def test_forward_is_the_step_runs_repeat_and_the_bag_form_is_the_user_table_form():
    rt, k = _rt(), make(130, 520, 32)
    ptr, items = fc.make_bags(dict(seed=5, B=130, NI=NI))
    res = []
    for form in ("bags", "bags", "table"):
        H, V, b = _tables(rt, dict(k, U=k["V"][::-1].copy()))
        net, opt = rt.SeqRec(H, V, b), rt.Optimizer.sgd(LR)
        if form == "bags":
            fwd = net.loss_sampled((ptr, items), k["pid"], k["cand"], **_kw(k))
            losses = net.step_sampled(opt, (ptr, items), k["pid"], k["cand"], **_kw(k, l2_reg=0.01))
        else:
            Q = net.user_table((ptr, items))
            uid = np.arange(130, dtype=np.int32)
            fwd = rt.sampled_softmax_loss(Q, V, b, uid, k["pid"], k["cand"], **_kw(k))
            losses = rt.sampled_softmax_step(opt, Q, V, b, uid, k["pid"], k["cand"], **_kw(k, l2_reg=0.01))
        assert np.array_equal(_bits(np.float32(fwd)), _bits(np.concatenate(losses)))      # the forward is the step's loss and l2
        res.append([_bits(V.read()), _bits(b.read()), _bits(np.concatenate(losses)), _bits(H.read())])
    assert all(np.array_equal(x, y) for x, y in zip(res[0], res[1]))                      # two runs, identical bits
    assert all(np.array_equal(x, y) for x, y in zip(res[0][:3], res[2][:3]))              # the item side, bit for bit
    assert not np.array_equal(res[0][0], _bits(k["V"]))


def test_the_bf16_loss_is_not_the_fp32_loss_and_adam_leaves_idle_rows_lazy():
    rt, k = _rt(), make(63, 65, 20)
    tabs, opt, kw = _tables(rt, k), rt.Optimizer.adam(fc.LR["adam"]), _kw(k)
    assert rt.sampled_softmax_loss(*tabs, k["uid"], k["pid"], k["cand"], **kw)[0] != \
        rt.sampled_softmax_loss(*tabs, k["uid"], k["pid"], k["cand"], **dict(kw, precision="fp32"))[0]
    rt.sampled_softmax_step(opt, *tabs, k["uid"], k["pid"], k["cand"], **kw)
    idle = np.setdiff1d(np.arange(NI), np.concatenate((k["pid"], k["cand"])))
    assert len(idle) > 5
    for t, W0 in ((tabs[1], k["V"]), (tabs[2], k["b"])):
        assert np.array_equal(_bits(t.read())[idle], _bits(W0)[idle]) and not np.array_equal(_bits(t.read()), _bits(W0))
        for slot in (0, 1):
            assert not _bits(np.asarray(opt.slot(t, slot)).reshape(W0.shape))[idle].any()


def test_an_unknown_precision_is_refused_by_all_four_calls():
    rt, k = _rt(), make(1, 1, 8)
    U, V, b = _tables(rt, k)
    net, bags, a = rt.SeqRec(rt.Table(NI, 8).write(k["V"]), V, b), (np.array([0, 1], np.int32), np.array([2], np.int32)), (k["pid"], k["cand"])
    for call in (lambda: rt.sampled_softmax_step(rt.Optimizer.sgd(LR), U, V, b, k["uid"], *a, precision="fp8"),
                 lambda: rt.sampled_softmax_loss(U, V, b, k["uid"], *a, precision="fp8"),
                 lambda: net.step_sampled(rt.Optimizer.sgd(LR), bags, *a, precision="fp8"),
                 lambda: net.loss_sampled(bags, *a, precision="fp8")):
        with pytest.raises(ValueError, match="precision"):
            call()
