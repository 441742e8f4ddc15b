"""The partial train step on the device against the fixtures minted from the REFERENCE'S OWN class text
(tests/golden/refstub/{bpr,ucml,wrmf}sub_*.npz, written by tests/golden/make_golden_subset.py: the reference's BPR / UCML / WRMF
with `tape.gradient` / `apply_gradients` on a subset of `model.trainable_variables`).  No oracle in between: the files go to the
HIP path through `rt.*_step(train=...)`.  Tolerances as tests/test_gpu_refstub.py: conftest.TOL, Adam conftest.TOL_ADAM; the
tables the reference left alone are bit-for-bit their inputs."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, TOL, TOL_ADAM, rel_err
from test_gpu_refstub import _make_opt

pytestmark = pytest.mark.gpu

REFSTUB = os.path.join(GOLDEN, "refstub")
ROLE = {"u": ("user", "U"), "i": ("item", "V"), "b": ("bias", "b")}


def _files():
    return sorted(f for f in os.listdir(REFSTUB) if "sub_" in f and f.endswith(".npz")) if os.path.isdir(REFSTUB) else []


def test_the_subset_fixtures_are_there():
    names = _files()
    assert 6 <= len(names) <= 10 and {n.split("sub_")[0] for n in names} == {"bpr", "ucml", "wrmf"}


@pytest.mark.parametrize("fname", _files())
def test_subset_step_on_the_device_matches_the_reference_text(fname):
    from openrec_amd import runtime as rt
    g = dict(np.load(os.path.join(REFSTUB, fname)))
    model, roles, _, optkind, _ = fname[:-4].split("_")
    model = model[:-3]
    assert roles == str(g["roles"])
    train = tuple(ROLE[r][0] for r in roles)
    tol = TOL_ADAM if optkind == "adam" else TOL
    tabs = {k: rt.Table(*g["in_" + k].shape).write(g["in_" + k]) for k in ("U", "V", "b")}
    opt = _make_opt(rt, optkind)
    losses = []
    for s in range(int(g["steps"])):
        uid, pid = np.roll(g["in_uid"], s), np.roll(g["in_pid"], 2 * s)
        if model == "wrmf":
            l, l2 = rt.pointwise_step("wrmf", opt, tabs["U"], tabs["V"], tabs["b"], None, uid, pid, np.roll(g["in_label"], s), a=2.0, b_w=0.5, train=train)
        else:
            l, l2 = rt.pairwise_step(model, opt, tabs["U"], tabs["V"], tabs["b"], uid, pid, np.roll(g["in_nid"], 3 * s), margin=0.5, train=train)
        losses.append((l[0], l2[0]))
    assert rel_err(np.array(losses, np.float64), g["losses"]) < tol
    trained = {ROLE[r][1] for r in roles}
    for k, t in tabs.items():
        if k in trained:
            assert rel_err(t.read(), g["out_" + k]) < tol, k
            for j, short in enumerate({"sgd": [], "adagrad": ["acc"], "adam": ["m", "v"]}[optkind]):
                assert rel_err(opt.slot(t, j), g["slot_%s_%s" % (k, short)]) < tol, (k, short)
        else:
            assert np.array_equal(g["out_" + k], g["in_" + k]), k          # the reference left it alone ...
            assert np.array_equal(t.read(), g["in_" + k]), k              # ... and so did the device, to the bit
