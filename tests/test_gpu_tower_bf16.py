"""GPU: the tower's layers with bf16 operands on the matrix cores (tower_precision="bf16", ORX_TOWER_BF16) against the rounded
semantics of include/openrec_hip.h in float64: bf(x) is a torch.bfloat16 round trip of the fp32 value, every sum is float64.  x0 is
taken from rt.bag_pool and the side rows, whose bits the tower's input launch has.

Forward bound.  Products of bf16 values are exact in fp32, so layer 1 differs from the float64 sum by fp32 accumulation alone:
TOL * m_1 + 1 ulp, m_{l+1} = m_l |bf(W_l)| + |c_l|, m_0 = |bf(x0)|.  From layer 2 on the device rounds ITS x_l to bf16: a value one
fp32 rounding away from a bf16 tie may round the other way, which moves it by one bf16 ulp, at most 2^-8 |x_l| <= 2^-8 m_l; through
|bf(W_l)| that is 2^-8 m_{l+1}, on top of the earlier layers' error carried the same way.  Layer l + 1: ((l + 1) TOL + l 2^-8) m_{l+1}.
Backward bound.  An operand pair (a, b) of a product contributes (2^-8 + TOL) |a| |b| -- 2^-9 for the rounding of a device value
that differs from the reference's in its last fp32 bits, doubled for the two operands; TOL is fp32 accumulation -- and the bound e
of the incoming gradient is carried through |bf(W_l)| and |bf(x_l)| beside it.  The l2 terms take TOL, the update 2 ulp."""
import numpy as np
import pytest
import torch

import fullsoftmax_ref as fr
from conftest import TOL, delta_check

pytestmark = pytest.mark.gpu
NI, K8 = 97, 2.0 ** -8
f64 = lambda x: np.asarray(x, np.float64)
ulp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)
bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.int32)


def bf(x):
    return f64(torch.from_numpy(np.ascontiguousarray(x, np.float32)).bfloat16().float().numpy())


def make(widths, m, bias, relu_last, seed, B=130):
    """-> (rt, net, the fp32 arrays by name, (bags, side ids, pid)); B = 130 bags: no multiple of the forward's tile, three dW chunks
    of one tile, the last one ragged; B = 2113, the smallest such B with two tiles per chunk: 17 chunks, the last tile one row.
    Bag 3 is empty.  Biases of +-0.5 against small products keep every masked pre-activation away from 0"""
    from openrec_amd import runtime as rt
    geo = rt.tower_geometry(B, widths, "bf16")
    assert B % geo["tile"] and geo["batch_chunks"] >= 2 and B % (64 * geo["tiles_per_chunk"]) and (geo["tiles_per_chunk"] >= 2) == (B > 130)
    rng = np.random.default_rng(seed)
    sd = [3, 4][:m]
    u = lambda r, d, a: rng.uniform(-a, a, (r, d)).astype(np.float32)
    A = dict(H=u(NI, widths[0] - sum(sd), 0.5), V=u(NI, widths[-1], 0.5), b=u(NI, 1, 0.5))
    A.update({f"S{j}": u(11, d, 0.5) for j, d in enumerate(sd)})
    for l in range(len(widths) - 1):
        A[f"W{l}"] = u(widths[l], widths[l + 1], 0.5 / widths[l])
        if bias:
            A[f"c{l}"] = (0.5 * np.where(rng.random((1, widths[l + 1])) < 0.5, -1, 1)).astype(np.float32)
    T = {k: rt.Table(*v.shape).write(v) for k, v in A.items()}
    L = len(widths) - 1
    net = rt.DeepSeqRec(T["H"], T["V"], T["b"], [(T[f"W{l}"], T.get(f"c{l}")) for l in range(L)], side=[T[f"S{j}"] for j in range(m)],
                        relu_last=relu_last)
    lens = rng.integers(1, 5, B); lens[3] = 0
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    lists = ((ptr, rng.integers(0, NI, ptr[-1]).astype(np.int32)), tuple(rng.integers(0, 11, B).astype(np.int32) for _ in range(m)),
             rng.integers(0, NI, B).astype(np.int32))
    return rt, net, A, T, lists


def x0_of(rt, net, A, lists):
    pool = rt.bag_pool(net.H, lists[0], rt.Table(len(lists[2]), net.H.dim)).read()
    return np.concatenate([A[f"S{j}"][f] for j, f in enumerate(lists[1])] + [pool], axis=1)


def forward(x0, A, L, relu_last):
    """-> activations, pre-activations, forward bounds (fp32 x0; float64 beyond)"""
    xs, zs, bounds, mag = [f64(x0)], [], [], np.abs(bf(x0))
    for l in range(L):
        Wb, c = bf(A[f"W{l}"]), f64(A.get(f"c{l}", 0.0))
        z = bf(xs[-1]) @ Wb + c
        mag = mag @ np.abs(Wb) + np.abs(c)
        bounds.append(((l + 1) * TOL + l * K8) * mag + ulp(mag))
        zs.append(z)
        xs.append(np.maximum(z, 0.0) if (l + 1 < L or relu_last) else z)
    return xs, zs, bounds


# ---- 1. exact anchor ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [50, 256])
def test_a_permutation_layer_gives_the_rounded_pool_bit_for_bit_in_any_batch(D):
    rt, net, A, T, (bags, _, _) = make([D, D], 0, False, False, seed=D)
    B = len(bags[0]) - 1
    perm = np.random.default_rng(D).permutation(D)
    P = np.zeros((D, D), np.float32); P[perm, np.arange(D)] = 1.0
    T["W0"].write(P)
    want = bf(rt.bag_pool(net.H, bags, rt.Table(B, D)).read())[:, perm].astype(np.float32)
    got = net.user_table(bags, tower_precision="bf16").read()
    assert np.array_equal(bits(got), bits(want)) and np.abs(want).max() > 0
    head = (bags[0][:66], bags[1][:bags[0][65]])
    assert np.array_equal(bits(net.user_table(head, out=rt.Table(65, D), tower_precision="bf16").read()), bits(want[:65]))


# ---- 2. forward against float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("widths,m,bias,relu_last", [([9, 50], 2, False, False), ([80, 256], 0, True, True), ([80, 256, 50, 9], 2, True, True),
                                                     ([50, 80, 256, 16], 0, True, False)])
def test_forward_is_the_float64_sum_of_the_rounded_operands(widths, m, bias, relu_last):
    rt, net, A, T, lists = make(widths, m, bias, relu_last, seed=len(widths) + widths[0])
    L = len(widths) - 1
    xs, _, bounds = forward(x0_of(rt, net, A, lists), A, L, relu_last)
    got = f64(net.user_table(lists[0], lists[1], tower_precision="bf16").read())
    err = np.abs(got - xs[-1])
    print(f"{widths}: worst element {(err / bounds[-1]).max():.3g} x bound")
    assert (err <= bounds[-1]).all()
    # the rounding is where the semantics put it: the unrounded tower is outside the fp32 path's tolerance of these outputs (the deep
    # cases have biases: without them three layers of random signs cancel to 1e-3 of the magnitude sum the tolerance is taken on)
    x, mag = f64(x0_of(rt, net, A, lists)), np.abs(f64(x0_of(rt, net, A, lists)))
    for l in range(L):
        c = f64(A.get(f"c{l}", 0.0))
        x, mag = x @ f64(A[f"W{l}"]) + c, mag @ np.abs(f64(A[f"W{l}"])) + np.abs(c)
        x = np.maximum(x, 0.0) if (l + 1 < L or relu_last) else x
    live = xs[-1] != 0
    outside = np.abs(got - x)[live] > (TOL * mag + ulp(mag))[live]
    print(f"{widths}: {outside.mean():.2f} of the elements outside the fp32 tolerance of the unrounded tower")
    assert outside.mean() > 0.5


# ---- 3. one SGD step with lr = 1: W0 - W1 is the gradient -----------------------------------------------------------------------
def ref_grads(rt, net, A, lists, L, relu_last, fs_bf16, scale, l2_reg, l2_mlp):
    """-> {table: (gradient, bound without the ulp term, or None for dc)}, and the margin min(|z| - forward bound) of the masked layers"""
    (ptr, items), side, pid = lists
    x0 = x0_of(rt, net, A, lists)
    xs, zs, fb = forward(x0, A, L, relu_last)
    masked = [l for l in range(L) if l + 1 < L or relu_last]
    margin = min([float((np.abs(zs[l]) - fb[l]).min()) for l in masked], default=1.0)
    V, b = f64(A["V"]), f64(A["b"])
    Qs, Vs = (bf(xs[-1]), bf(V)) if fs_bf16 else (xs[-1], V)
    a, _ = fr.coefficients(Qs, Vs, b, pid, None, None, scale)
    g = scale * (bf(a) if fs_bf16 else a) @ Vs
    # the softmax's own error and, below more than one layer, (first order) that of the coefficients under the forward bound of the
    # query; a single layer has no rounded value upstream and keeps the pure (2^-8 + TOL) sum |a| |b| terms
    dq = fb[-1] + (K8 * np.abs(xs[-1]) if fs_bf16 else 0.0)              # (bf16 softmax: the device rounds ITS query)
    first = 2 * scale * (dq @ np.abs(Vs).T).max(1, keepdims=True) if L > 1 else 0.0
    e = ((K8 if fs_bf16 else 0.0) + TOL + first) * scale * np.abs(a) @ np.abs(Vs)
    k, out = K8 + TOL, {}
    for l in reversed(range(L)):
        if l in masked:
            g, e = g * (xs[l + 1] > 0), e * (xs[l + 1] > 0)
        W, Wb, xb, ex = f64(A[f"W{l}"]), bf(A[f"W{l}"]), bf(xs[l]), (fb[l - 1] if l else 0.0 * xs[0])
        out[f"W{l}"] = (xb.T @ bf(g) + l2_mlp * W, k * np.abs(xb).T @ np.abs(g) + (np.abs(xb) + ex).T @ e + ex.T @ np.abs(g) + TOL * l2_mlp * np.abs(W))
        if f"c{l}" in A:
            out[f"c{l}"] = (g.sum(0)[None, :] + l2_mlp * f64(A[f"c{l}"]), None)
        g, e = bf(g) @ Wb.T, (k * np.abs(g) + e) @ np.abs(Wb).T
    g, e = g + l2_reg * f64(x0), e + TOL * l2_reg * np.abs(f64(x0))
    c0 = 0
    for j, f in enumerate(side):
        d = A[f"S{j}"].shape[1]
        G, E = np.zeros(A[f"S{j}"].shape), np.zeros(A[f"S{j}"].shape)
        np.add.at(G, f, g[:, c0:c0 + d]); np.add.at(E, f, e[:, c0:c0 + d] + TOL * np.abs(g[:, c0:c0 + d]))
        out[f"S{j}"], c0 = (G, E), c0 + d
    own = np.repeat(np.arange(len(pid)), np.diff(ptr))
    ci = 1.0 / np.maximum(np.diff(ptr), 1)[own, None]
    G, E = np.zeros(A["H"].shape), np.zeros(A["H"].shape)
    np.add.at(G, items, ci * g[own, c0:]); np.add.at(E, items, ci * (e[own, c0:] + TOL * np.abs(g[own, c0:])))
    out["H"] = (G, E)
    return out, margin


CASES = [([9, 50], 2, False, False, "fp32", "host", 130), ([80, 256], 0, True, True, "bf16", "device", 130),
         ([80, 256, 50, 9], 2, True, True, "fp32", "device", 130), ([50, 80, 256, 16], 0, True, False, "bf16", "host", 130),
         ([80, 256, 50, 9], 2, True, True, "fp32", "sets", 130),
         # two tiles per dW chunk: the prefetch, the accumulators and dc carried over tiles, a ragged last chunk.  (The biased case is
         # 16 wide: at 256 the bias-dominated queries are nearly equal and |s| ~ 10, the fp32 softmax's score rounding then moves every
         # row's coefficients the same way by 1e-6, and 2113 rows of that are 4 ulp of c_0 -- 1.6 x delta_check, from outside the tower.)
         ([9, 50], 2, False, False, "fp32", "host", 2113), ([80, 16], 0, True, True, "fp32", "device", 2113)]


@pytest.mark.parametrize("widths,m,bias,relu_last,precision,where,B", CASES)
def test_one_sgd_step_gives_the_gradients_of_the_rounded_semantics(widths, m, bias, relu_last, precision, where, B):
    rt, net, A, T, lists = make(widths, m, bias, relu_last, seed=7 + widths[1], B=B)
    scale, l2_reg, l2_mlp = 2.0, float(np.float32(0.01)), float(np.float32(0.02))
    want, margin = ref_grads(rt, net, A, lists, len(widths) - 1, relu_last, precision == "bf16", scale, l2_reg, l2_mlp)
    assert margin > 0, "a masked pre-activation of the reference lies within the forward bound of 0: another seed"
    dev = (lambda x: torch.from_numpy(x).cuda()) if where == "device" else (lambda x: x)
    bags, side, pid = (dev(lists[0][0]), dev(lists[0][1])), tuple(dev(f) for f in lists[1]), dev(lists[2])
    kw = dict(scale=scale, l2_reg=l2_reg, l2_mlp=l2_mlp, tower_precision="bf16")
    if where == "sets":                         # sets of one with t = 1 are the single-label objective
        net.step_full(rt.Optimizer.sgd(1.0), bags, None, side, labels=(np.arange(B + 1, dtype=np.int32), pid), **kw)
    else:
        net.step_full(rt.Optimizer.sgd(1.0), bags, pid, side, precision=precision, **kw)
    for name, (grad, bound) in want.items():
        W0, got = A[name], T[name].read()
        new = f64(W0) - grad
        if bound is None:                       # dc sums the unrounded gm: the fp32 path's check
            delta_check(W0, got, new.astype(np.float32), what=name)
            continue
        u = np.spacing(np.maximum(np.maximum(np.abs(new), np.abs(W0)), np.abs(grad).max()).astype(np.float32)).astype(np.float64)
        err = np.abs(f64(got) - new)
        print(f"{widths} B={B} {name}: worst element {(err / (bound + 2 * u)).max():.3g} x bound")
        assert (err <= bound + 2 * u).all(), name
        assert not np.array_equal(got, W0)


def test_one_adam_step_fills_the_slots_from_the_gradients_of_the_rounded_semantics():
    widths, relu_last = [80, 256, 50, 9], True
    rt, net, A, T, lists = make(widths, 2, True, relu_last, seed=263)
    want, margin = ref_grads(rt, net, A, lists, 3, relu_last, False, 1.0, 0.0, 0.0)
    assert margin > 0
    lr, b1, b2, eps = 2e-3, 0.9, 0.999, 1e-7
    opt = rt.Optimizer.adam(lr, b1, b2, eps)
    net.step_full(opt, lists[0], lists[2], lists[1], train=("tower",), tower_precision="bf16")
    for l in range(3):
        g, bound = want[f"W{l}"]
        m, v = opt.slot(T[f"W{l}"], 0), opt.slot(T[f"W{l}"], 1)
        assert (np.abs(f64(m) - (1 - b1) * g) <= (1 - b1) * bound + 2 * ulp(m)).all() and np.abs(m).max() > 0
        assert (np.abs(f64(v) - (1 - b2) * g * g) <= (1 - b2) * (2 * np.abs(g) * bound + bound ** 2) + 2 * ulp(v)).all()
        assert not np.array_equal(T[f"W{l}"].read(), A[f"W{l}"])


# ---- 4. consistency ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_forward_is_the_steps_loss_two_runs_agree_fp32_keeps_its_bits_and_masks_hold(precision):
    widths = [80, 256, 50, 9]
    runs = {}
    for tp in ("bf16", "bf16", "fp32", None):
        rt, net, A, T, (bags, side, pid) = make(widths, 2, True, True, seed=5)
        kw = dict(precision=precision, **({} if tp is None else {"tower_precision": tp}))
        fwd = net.loss_full(bags, pid, side, **kw)
        loss, l2 = net.step_full(rt.Optimizer.sgd(0.05), bags, pid, side, l2_reg=0.01, l2_mlp=0.01, **kw)
        assert bits(np.float32(fwd[0])) == bits(loss)[0] and bits(np.float32(fwd[1])) == bits(l2)[0]
        runs.setdefault(tp, []).append([bits(t.read()) for t in T.values()] + [bits(loss), bits(l2), bits(net.user_table(bags, side, **({} if tp is None else {'tower_precision': tp})).read())])
    assert all(np.array_equal(x, y) for x, y in zip(*runs["bf16"]))
    assert all(np.array_equal(x, y) for x, y in zip(runs["fp32"][0], runs[None][0]))
    assert not all(np.array_equal(x, y) for x, y in zip(runs["bf16"][0], runs["fp32"][0]))
    rt, net, A, T, (bags, side, pid) = make(widths, 2, True, True, seed=5)
    net.step_full(rt.Optimizer.sgd(0.05), bags, pid, side, train=("history", "item"), precision=precision, tower_precision="bf16")
    assert all(np.array_equal(bits(T[f"W{l}"].read()), bits(A[f"W{l}"])) for l in range(3)) and not np.array_equal(T["H"].read(), A["H"])


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from openrec_amd import _ffi
    rt, net, A, T, (bags, side, pid) = make([9, 50], 2, False, False, seed=1)
    B = len(pid)
    with pytest.raises(ValueError, match="tower_precision"):
        net.user_table(bags, side, tower_precision="fp8")
    with pytest.raises(ValueError, match="tower_precision"):
        net.step_full(rt.Optimizer.sgd(0.05), bags, pid, side, tower_precision="fp8")
    ctx, sgd, (ptr, ids) = net.ctx, rt.Optimizer.sgd(0.05), bags
    H2 = rt.Table(NI, 50).write(np.zeros((NI, 50), np.float32))
    with pytest.raises(ValueError, match="orx_seqrec_full_step: ORX_TOWER_BF16"):
        _ffi.check(ctx._lib.orx_seqrec_full_step(ctx._h, sgd._h, H2._h, T["V"]._h, None, ptr.ctypes.data, ids.ctypes.data, pid.ctypes.data, None, None,
                                                 B, len(ids), _ffi.ORX_BAG_MEAN, 1.0, 1.0, 0.0, 0, 0, 0, _ffi.ORX_TOWER_BF16, None, None))
    model, arrays = net._model_args([f.ctypes.data for f in side])
    with pytest.raises(ValueError, match="orx_tower_sets_step: ORX_FS_BF16"):
        _ffi.check(ctx._lib.orx_tower_sets_step(ctx._h, sgd._h, T["H"]._h, T["V"]._h, None, *model, ptr.ctypes.data, ids.ctypes.data, ptr.ctypes.data,
                                                ids.ctypes.data, None, len(ids), None, None, B, len(ids), _ffi.ORX_BAG_MEAN, 1.0, 1.0, 0.0, 0.0, 0, 0, 0,
                                                _ffi.ORX_FS_BF16 | _ffi.ORX_TOWER_BF16, None, None))
