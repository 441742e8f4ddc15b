"""The seeded cases of the tower step shared by tests/test_tower_cpu.py (the reference against autograd, float32 against float64)
and tests/test_gpu_tower.py (the device against the float64 reference).

The shapes -- side tables (rows, dim), Dh, the layers' output widths, which layers have a bias, relu_last, item bias, B, NI,
chunk_items, chunk_samples:
    wide-in    (2, 3) (37, 5)   50   70 50       c c    relu   b    130  300  128  64   in_0 = 3 + 5 + 50 = 58 -> 70 -> 50, no width on a
                                                                                        tile edge; the 2-row side table: every sample
                                                                                        repeats; three batch tiles; forced chunks (3, 3)
    widest     -               256   256         -      relu   -     65   40    0  64   256 -> 256; no side table and no bias: the empty
                                                                                        bag 0 has pre-activations that are exactly 0
    one-wide   -                 4   1 6         c -    lin    b     64   40    0   0   a 1-wide hidden layer; exactly one batch tile
    three      (2, 8) (100, 8)  16   33 20 12    - c c  relu   b      1   40    0   0   L = 3; a single sample
    linear     -                24   24          c      lin    -     65  300    0   0   L = 1, the last layer linear; one row past a tile
Every optimizer meets every shape: 20 cases.  Bags are fullsoftmax_cases.make_bags' (bag 0 empty where B > 1).

The relu margin.  A relu whose pre-activation is within rounding of 0 makes two correct implementations disagree by a whole
term, so a case's data is drawn from the first seed in (seed, seed + 7919, ...) whose float64 pre-activations all satisfy
    |z_ij| > 64 u sum_k |x_ik W_kj|,    u = 2^-24
-- `make` asserts it -- except pre-activations that are exactly 0 in float64 AND in float32 (an empty bag without side rows under
a zero bias), which stay in and test relu'(0) = 0.  No element is ever left out of a comparison."""
import numpy as np

import fullsoftmax_cases as fc
import tower_ref as tr

OPTS, LR, SCALE = fc.OPTS, fc.LR, fc.SCALE
U32 = 2.0 ** -24

#        name        side (rows, dim)        Dh   outs          bias of layer          relu_last  b      B    NI   ci   cs
SHAPES = (("wide-in", ((2, 3), (37, 5)), 50, (70, 50), (True, True), True, True, 130, 300, 128, 64),
          ("widest", (), 256, (256,), (False,), True, False, 65, 40, 0, 64),
          ("one-wide", (), 4, (1, 6), (True, False), False, True, 64, 40, 0, 0),
          ("three", ((2, 8), (100, 8)), 16, (33, 20, 12), (False, True, True), True, True, 1, 40, 0, 0),
          ("linear", (), 24, (24,), (True,), False, False, 65, 300, 0, 0))
# (item chunks, sample chunks) of the full softmax under the forced chunk arguments
FORCED_CHUNKS = {0: (3, 3), 1: (1, 2)}


def shape_case(si, opt="sgd", seed=None):
    name, side, Dh, outs, cb, relu_last, bias, B, NI, ci, cs = SHAPES[si]
    return dict(name=f"{opt}-{name}", opt=opt, shape=si, side=side, Dh=Dh, outs=outs, cbias=cb, relu_last=relu_last, bias=bias, B=B, NI=NI,
                chunk_items=ci, chunk_samples=cs, seed=7000 + si if seed is None else seed)


CASES = [shape_case(si, opt, seed=7000 + 8 * oi + si) for oi, opt in enumerate(OPTS) for si in range(len(SHAPES))]


def widths(case):
    return (sum(d for _, d in case["side"]) + case["Dh"],) + tuple(case["outs"])


def _draw(case, seed):
    rng = np.random.default_rng(seed)
    B, NI, Dh = case["B"], case["NI"], case["Dh"]
    w = widths(case)
    u = lambda *shape: rng.uniform(-SCALE, SCALE, shape).astype(np.float32)
    H, V, b = u(NI, Dh), u(NI, w[-1]), u(NI, 1)
    S = [u(r, d) for r, d in case["side"]]
    layers = []
    for l, has_c in enumerate(case["cbias"]):
        a = np.sqrt(6.0 / (w[l] + w[l + 1]))
        W = rng.uniform(-a, a, (w[l], w[l + 1])).astype(np.float32)
        layers.append([W, rng.uniform(-0.1, 0.1, (1, w[l + 1])).astype(np.float32) if has_c else None])
    f = [rng.integers(0, r, B).astype(np.int32) for r, _ in case["side"]]
    pid = rng.integers(0, NI, B).astype(np.int32)
    ptr, items = fc.make_bags(dict(seed=seed, B=B, NI=NI))
    return dict(H=H, V=V, b=b if case["bias"] else None, S=S, layers=layers, f=f, pid=pid, ptr=ptr, items=items)


def f64(x):
    if x is None:
        return None
    if isinstance(x, (list, tuple)):
        return [f64(y) for y in x]
    return np.asarray(x).astype(np.float64)


def margin_ok(m, relu_last, pool="mean"):
    """the relu-margin condition of the module's docstring on the model m (float32 tables)"""
    x0, _, _ = tr.input_rows(m["H"], m["S"], m["ptr"], m["items"], m["f"], pool)
    x32, z32 = tr.tower(x0, m["layers"], relu_last)
    x0d, _, _ = tr.input_rows(f64(m["H"]), f64(m["S"]), m["ptr"], m["items"], m["f"], pool)
    l64 = f64(m["layers"])
    x64, z64 = tr.tower(x0d, l64, relu_last)
    for l, (W, _) in enumerate(l64):
        if not (l + 1 < len(l64) or relu_last):
            continue
        T = np.abs(x64[l]) @ np.abs(W)
        zero = (z64[l] == 0) & (z32[l] == 0)
        if not ((np.abs(z64[l]) > 64 * U32 * T) | zero).all():
            return False
    return True


def make(case, pool="mean"):
    """-> the model and the lists of the case: dict(H, V, b, S, layers, f, pid, ptr, items), float32 / int32"""
    for k in range(64):
        m = _draw(case, case["seed"] + 7919 * k)
        if margin_ok(m, case["relu_last"], pool):
            return m
    raise AssertionError(f"{case['name']}: no seed with the relu margin")


def copy_model(m, dtype=None):
    c = (lambda x: None if x is None else (x.copy() if dtype is None else x.astype(dtype)))
    return dict(m, H=c(m["H"]), V=c(m["V"]), b=c(m["b"]), S=[c(s) for s in m["S"]], layers=[[c(W), c(cl)] for W, cl in m["layers"]])


def make_opt(name):
    return fc.make_opt(name)
