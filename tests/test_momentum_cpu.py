"""SGD with momentum / Nesterov (keras.optimizers.SGD(momentum > 0)): the host-only pieces -- the NumPy restatement the GPU
tests compare against (tests/keras_momentum.py) pinned by a hand-computed case, the compat optimizer's construction and
validation, and the C ABI's kind value.  No device is touched."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from keras_momentum import Momentum


def _hand(nesterov):
    """three steps on a 4 x 2 table, duplicate ids, written out element by element in float64"""
    lr, m = 0.1, 0.9
    w = [[1.0, -1.0], [0.5, 0.25], [2.0, 0.0], [-0.5, 1.5]]
    a = [[0.0, 0.0] for _ in range(4)]
    steps = [
        ([0, 2, 0], [[1.0, 2.0], [0.5, -0.5], [3.0, -1.0]]),        # row 0 twice
        ([1, 1, 1], [[0.25, 0.0], [0.25, 1.0], [0.5, -1.0]]),       # row 1 three times, rows 0 and 2 keep their velocity
        ([0, 3], [[-1.0, 1.0], [2.0, 2.0]]),
    ]
    for ids, gs in steps:
        G = {}
        for r, g in zip(ids, gs):
            G.setdefault(r, [0.0, 0.0])
            G[r] = [G[r][0] + g[0], G[r][1] + g[1]]
        for r, g in G.items():
            for e in range(2):
                a[r][e] = a[r][e] * m - lr * g[e]
                w[r][e] += (a[r][e] * m - lr * g[e]) if nesterov else a[r][e]
    return np.array(w), np.array(a), steps


@pytest.mark.parametrize("nesterov", [False, True])
def test_restatement_matches_a_hand_computed_three_step_case(nesterov):
    want_w, want_a, steps = _hand(nesterov)
    var = np.array([[1.0, -1.0], [0.5, 0.25], [2.0, 0.0], [-0.5, 1.5]], np.float32)
    opt = Momentum(0.1, 0.9, nesterov)
    for ids, gs in steps:
        opt.apply(var, np.array(ids), np.array(gs, np.float32), key="t")
    assert np.allclose(var, want_w, rtol=1e-6, atol=1e-6)
    assert np.allclose(opt.vel["t"], want_a, rtol=1e-6, atol=1e-6)
    # the dense rule is the same rule on every element
    d = np.array([1.0, -2.0, 0.5], np.float32)
    od = Momentum(0.1, 0.9, nesterov)
    for g in ([1.0, 1.0, 1.0], [0.0, -1.0, 2.0]):
        od.apply_dense(d, np.array(g, np.float32), key="d")
    a1 = -0.1 * np.array([1.0, 1.0, 1.0])
    a2 = a1 * 0.9 - 0.1 * np.array([0.0, -1.0, 2.0])
    step = (lambda a, g: a * 0.9 - 0.1 * g) if nesterov else (lambda a, g: a)
    want = np.array([1.0, -2.0, 0.5]) + step(a1, np.ones(3)) + step(a2, np.array([0.0, -1.0, 2.0]))
    assert np.allclose(d, want, rtol=1e-6, atol=1e-6) and np.allclose(od.vel["d"], a2, rtol=1e-6, atol=1e-7)


def test_restatement_plain_form_is_the_nesterov_expression_with_unit_coefficients():
    # w += a*c1 - c2*G with (c1, c2) = (1, 0) is bit-exact w += a (the kernels use that one expression for both forms)
    rng = np.random.default_rng(3)
    w = rng.standard_normal(1000).astype(np.float32)
    a = rng.standard_normal(1000).astype(np.float32)
    G = rng.standard_normal(1000).astype(np.float32)
    one, zero = np.float32(1.0), np.float32(0.0)
    assert np.array_equal(w + (a * one - zero * G), w + a)


def test_compat_sgd_with_momentum_constructs_without_a_device():
    from openrec_amd.tf2 import compat
    opt = compat.SGD(0.01, momentum=0.9, nesterov=True)
    assert opt.momentum == pytest.approx(0.9) and opt.nesterov is True and opt.learning_rate == pytest.approx(0.01)
    assert opt._native is None                       # nothing native until the first step
    plain = compat.SGD(learning_rate=0.05, momentum=0.5)
    assert plain.momentum == pytest.approx(0.5) and plain.nesterov is False


@pytest.mark.parametrize("bad", [1.5, -0.1, float("nan")])
def test_compat_sgd_rejects_momentum_outside_unit_interval(bad):
    from openrec_amd.tf2 import compat
    with pytest.raises(ValueError):
        compat.SGD(momentum=bad)


def test_compat_sgd_without_momentum_keeps_the_plain_sgd_kind(monkeypatch):
    from openrec_amd import runtime as rt
    from openrec_amd.tf2 import compat
    made = []
    monkeypatch.setattr(rt.Optimizer, "sgd", classmethod(lambda cls, lr=0.01, ctx=None: made.append(("sgd", lr)) or "sgd"))
    monkeypatch.setattr(rt.Optimizer, "momentum",
                        classmethod(lambda cls, lr=0.01, momentum=0.9, nesterov=False, ctx=None: made.append(("momentum", lr, momentum, nesterov)) or "mom"))
    assert compat.SGD(0.05, momentum=0)._make(None) == "sgd"
    assert compat.SGD(0.05)._make(None) == "sgd"
    assert compat.SGD(0.05, momentum=0.9, nesterov=True)._make(None) == "mom"
    assert made == [("sgd", 0.05), ("sgd", 0.05), ("momentum", 0.05, 0.9, True)]


def test_ffi_momentum_kind_matches_the_header():
    from openrec_amd import _ffi
    from openrec_amd import runtime as rt
    hdr = open(os.path.join(ROOT, "include", "openrec_hip.h")).read()
    enum = re.search(r"enum orx_opt_kind \{([^}]*)\}", hdr).group(1)
    vals = {k: int(v) for k, v in re.findall(r"(ORX_\w+)\s*=\s*(\d+)", enum)}
    assert vals["ORX_MOMENTUM"] == 3 and _ffi.ORX_MOMENTUM == 3
    assert rt.Optimizer.KINDS["momentum"] == _ffi.ORX_MOMENTUM
