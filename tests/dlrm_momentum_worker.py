"""Worker of test_gpu_momentum.py::test_dlrm_momentum_fp16_mlp_mode: DLRM in fp16-MLP mode with SGD momentum (plain and Nesterov)
against the fp16-operand DLRMOracle driven by tests/keras_momentum.py.  One process per environment variant (the DLRM switches
are read once per process).  The fp16 mode takes the fused dense optimizer launch, which carries the sorted sparse apply's
finish pass unless ORX_DLRM_FINISH_LAUNCH=1; ORX_DLRM_NO_FUSED_DENSE=1 takes the multi-tensor dense apply instead.

(1) step by step, every step from the oracle's parameters AND velocities: loss and every update within test_gpu_dlrm.py's fp16
bounds (dlrm_util.assert_fp16_updates); (2) free-running, four steps twice: bit-identical, and first-order faithful.
Prints "OK" and exits 0 when every check holds."""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from openrec_amd import runtime as rt  # noqa: E402
from oracle.dlrm_oracle import DLRMOracle  # noqa: E402
from dlrm_util import (assert_fp16_updates, assert_same_bits, assert_updates, draw_batch, load_model, params_of,  # noqa: E402
                       round_to_fp32, snapshot)
from keras_momentum import Momentum  # noqa: E402

TOL_FP16, TOL_FP16_EMB = 1e-4, 1.5e-3          # test_gpu_dlrm.py's bounds of the fp16-MLP mode
LR, MOM = 0.02, 0.9


def set_velocity(m, o, opt, vel):
    """the restatement's velocities (absent: zero) into the device optimizer's slot 0"""
    emb = [np.asarray(vel.get(("emb", f), np.zeros_like(o.emb[f]))) for f in range(len(o.emb))]
    opt.set_slot(m.param("emb"), np.concatenate(emb).astype(np.float32))
    for nm, layers in (("bot", o.bot), ("top", o.top)):
        for l, (W, b) in enumerate(layers):
            opt.set_slot(m.param(nm + "_w", l), np.asarray(vel.get((nm, l, "W"), np.zeros_like(W)), np.float32))
            opt.set_slot(m.param(nm + "_b", l), np.asarray(vel.get((nm, l, "b"), np.zeros_like(b)), np.float32).reshape(1, -1))


def run(nesterov):
    rng = np.random.default_rng(11)
    ln_emb = [50, 300, 7, 1000, 33]                   # a 7-row table: rows referenced by hundreds of lookups (the finish pass)
    cfg = dict(m_spa=32, ln_bot=[96, 32], ln_top=[200, 72, 1], dense_dim=13, ln_emb=ln_emb)
    B_full = 333
    o = DLRMOracle(dtype=np.float64, operand_dtype=np.float16, seed=5, reference_compat=False, **cfg)
    for W, b in o.bot + o.top:
        b[:] = rng.normal(size=b.shape) * 0.1
    round_to_fp32(o)
    oo = Momentum(LR, MOM, nesterov)
    batches, ref, states, vels = [], [], [copy.deepcopy(o)], [{}]
    for step in range(4):
        B = (B_full, B_full // 2 + 3, B_full // 5 + 1, B_full)[step]
        bt = draw_batch(o, rng, B, ln_emb, label_p=0.3, dense_dim=cfg["dense_dim"])
        batches.append(bt); ref.append(o.step(*bt, oo))
        round_to_fp32(o)
        for k in oo.vel:                              # the device holds its velocities in fp32 too
            oo.vel[k][...] = oo.vel[k].astype(np.float32)
        states.append(copy.deepcopy(o)); vels.append(copy.deepcopy(oo.vel))
    kw = dict(reference_compat=False, fp16_mlp=True)
    # ---- (2) free-running, twice
    start = {k: v.astype(np.float32) for k, v in params_of(states[0]).items()}
    snaps = []
    for _ in range(2):
        m = rt.DLRMModel(**cfg, **kw)
        load_model(m, states[0])
        opt = rt.Optimizer.momentum(LR, MOM, nesterov)
        losses = [m.step(opt, *bt)[0] for bt in batches]
        snaps.append((np.array(losses), snapshot(m, states[0], opt)))
    assert_same_bits(snaps[0][1], snaps[1][1])
    assert np.array_equal(snaps[0][0], snaps[1][0])
    assert_updates(start, snaps[0][1], params_of(o), 1e-2 + 16.0 / B_full, what=f"nesterov={nesterov} free-running", steps=4,
                   tol_of={"emb": 0.2})
    # ---- (1) strict, every step from the oracle's parameters and velocities
    m = rt.DLRMModel(**cfg, **kw)
    opt = rt.Optimizer.momentum(LR, MOM, nesterov)
    for step, bt in enumerate(batches):
        load_model(m, states[step])
        set_velocity(m, states[step], opt, vels[step])
        before = {k: v.astype(np.float32) for k, v in params_of(states[step]).items()}
        loss = m.step(opt, *bt)[0]
        assert abs(loss - ref[step]) <= TOL_FP16 * abs(ref[step]), (step, loss, ref[step])
        assert_fp16_updates(before, snapshot(m, o), params_of(states[step + 1]), len(bt[2]), len(ln_emb), TOL_FP16, TOL_FP16_EMB,
                            what=f"nesterov={nesterov} step {step}")


if __name__ == "__main__":
    for nesterov in (False, True):
        run(nesterov)
    print("OK")
