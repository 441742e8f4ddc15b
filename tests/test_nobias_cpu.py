"""The bias-free BPR fixtures (tests/golden/refstub/bprnb_*.npz, minted by tests/golden/make_golden_nobias.py from the reference's
LatentFactor and PairwiseLogLoss without biases) against the restatement the GPU tests use: a step of the biased oracle on a bias
table that is all zero when the step starts.  CPU only."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, OPT_KW, rel_err
from oracle import numpy_oracle as orc

REFSTUB = os.path.join(GOLDEN, "refstub")
REFERENCE = "/root/reference"


def fixtures():
    return sorted(f for f in os.listdir(REFSTUB) if f.startswith("bprnb_") and f.endswith(".npz"))


def make_opt(kind):
    return {"sgd": orc.SGD, "adagrad": orc.Adagrad, "adam": orc.AdamTFSparse}[kind](**OPT_KW[kind])


def restated(g, optkind, dtype):
    U, V = (g["in_" + k].astype(dtype) for k in ("U", "V"))
    bz = np.zeros((V.shape[0], 1), dtype)
    opt = make_opt(optkind)
    losses = []
    for s in range(int(g["steps"])):
        uid, pid, nid = np.roll(g["in_uid"], s), np.roll(g["in_pid"], 2 * s), np.roll(g["in_nid"], 3 * s)
        losses.append(orc.bpr_step(U, V, bz, uid, pid, nid, opt))
        bz[:] = 0
    return np.array(losses, np.float64), U, V, opt


def test_the_fixtures_are_there_and_small():
    names = fixtures()
    assert names == sorted("bprnb_d%d_%s_s0.npz" % (D, ok) for D in (50, 64) for ok in ("sgd", "adagrad", "adam"))
    for f in names:
        assert os.path.getsize(os.path.join(REFSTUB, f)) < 100 * 1024
        g = np.load(os.path.join(REFSTUB, f))
        assert not any(k.endswith("_b") or "_b_" in k or k == "grad0_b" for k in g.files), f


@pytest.mark.parametrize("fname", fixtures())
@pytest.mark.parametrize("dtype,tol", [(np.float64, 2e-7), (np.float32, 1e-5)])
def test_fixtures_agree_with_the_zero_bias_restatement(fname, dtype, tol):
    g = np.load(os.path.join(REFSTUB, fname))
    optkind = fname.split("_")[2]
    losses, U, V, opt = restated(g, optkind, dtype)
    if optkind == "adam":
        tol = max(tol, 5e-5 if dtype == np.float32 else tol)
    assert rel_err(losses, g["losses"]) < tol
    assert rel_err(U, g["out_U"]) < tol and rel_err(V, g["out_V"]) < tol
    slots = {"adagrad": lambda: [("acc", opt.acc)], "adam": lambda: [("m", opt.m), ("v", opt.v)]}.get(optkind, list)()
    for short, store in slots:
        for k in ("U", "V"):
            assert rel_err(store[k], g["slot_%s_%s" % (k, short)]) < tol, (short, k)


def test_minting_a_case_reproduces_the_committed_file():
    if not os.path.isdir(os.path.join(REFERENCE, "openrec", "tf2")):
        pytest.skip("the reference tree is not on this machine")
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        # (a process of its own: the stub backend installs stand-in `tensorflow` / `openrec` modules)
        subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_nobias.py"), "--backend", "stub", "--reference", REFERENCE,
                        "--out", d, "--only", "d50_sgd"], check=True, capture_output=True, timeout=600)
        fn = os.path.join(d, "bprnb_d50_sgd_s0.npz")
        new, old = np.load(fn), np.load(os.path.join(REFSTUB, os.path.basename(fn)))
        assert sorted(new.files) == sorted(old.files)
        for k in new.files:
            if k != "backend":
                assert np.array_equal(new[k], old[k]), k
