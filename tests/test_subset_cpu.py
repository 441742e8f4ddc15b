"""The partial train step, as far as it can be checked without a device: the two entry points are declared, exported and
typed; the mask constants; the runtime refuses a bad `train` before any device call; `LatentFactor.trainable`."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _header():
    return open(os.path.join(ROOT, "include", "openrec_hip.h")).read()


def _decl_arity(name):
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S)
    assert m, f"{name} is not declared in openrec_hip.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name,full", [("orx_pairwise_step_subset", "orx_pairwise_step"), ("orx_pointwise_step_subset", "orx_pointwise_step")])
def test_entry_points_are_declared_exported_and_typed(name, full):
    from openrec_amd import _ffi
    lib = _ffi.load()
    assert hasattr(lib, name)
    res, args = _ffi.SIGNATURES[name]
    _, full_args = _ffi.SIGNATURES[full]
    assert res is _ffi.c_int
    # the arguments of the full step with the mask in front of the two outputs
    assert len(args) == len(full_args) + 1 == _decl_arity(name) and _decl_arity(full) == len(full_args)
    assert args[:-3] == full_args[:-2] and args[-3] is _ffi.c_int and args[-2:] == full_args[-2:]


def test_mask_constants():
    from openrec_amd import _ffi
    assert (_ffi.ORX_TRAIN_USER, _ffi.ORX_TRAIN_ITEM, _ffi.ORX_TRAIN_BIAS) == (1, 2, 4)
    m = re.search(r"enum\s+orx_train_mask\s*\{(.*?)\}", _header(), flags=re.S)
    vals = dict((k.strip(), int(v)) for k, v in (e.split("=") for e in m.group(1).split(",")))
    assert vals == {"ORX_TRAIN_USER": 1, "ORX_TRAIN_ITEM": 2, "ORX_TRAIN_BIAS": 4}


from runtime_standin import NoDevice as _NoDevice          # (any use of it is a device call the check should have come before)


@pytest.mark.parametrize("train,bias,word", [(("users",), "t", "unknown"), ((), "t", "empty"), (("user", "bias"), None, "bias"), ("all", "t", "unknown")])
def test_runtime_refuses_a_bad_train_before_any_device_call(train, bias, word):
    from openrec_amd import runtime as rt
    t = _NoDevice()
    ids = np.zeros(4, np.int32)
    bias_t = None if bias is None else t
    with pytest.raises(ValueError, match=word):
        rt.pairwise_step("bpr", t, t, t, bias_t, ids, ids, ids, train=train)
    with pytest.raises(ValueError, match=word):
        rt.pointwise_step("wrmf", t, t, t, bias_t, None, ids, ids, ids.astype(np.float32), train=train)


def test_train_mask_values():
    from openrec_amd import runtime as rt
    assert rt._train_mask(None, object()) is None
    assert rt._train_mask(("user",), None) == 1 and rt._train_mask("item", None) == 2
    assert rt._train_mask(["bias", "user"], object()) == 5 and rt._train_mask(("user", "item", "bias"), object()) == 7


def test_latent_factor_trainable_toggles_trainable_variables():
    """LatentFactor allocates a device table in its constructor: the property logic is checked on an instance made without it"""
    from openrec_amd.tf2.modules.latent_factor import LatentFactor, Variable
    from openrec_amd.tf2.recommenders._base import Recommender
    lfs = []
    for name in ("user", "item", "bias"):
        lf = LatentFactor.__new__(LatentFactor)
        lf.table = object()
        lf._var = Variable(lf.table, name)
        lfs.append(lf)
    u, i, b = lfs
    assert u.trainable is True and u.trainable_variables == [u._var] == u.variables
    m = Recommender.__new__(Recommender)
    m.user_latent_factor, m.item_latent_factor, m.item_bias = u, i, b
    assert m.trainable_variables == [u._var, i._var, b._var] == m.variables
    i.trainable = False
    assert i.trainable_variables == [] and i.variables == [i._var]
    assert m.trainable_variables == [u._var, b._var] and m.variables == [u._var, i._var, b._var]
    # the roles apply_gradients derives from a variable list, by table identity
    assert m._train_roles(m.trainable_variables) == ("user", "bias")
    assert m._train_roles(m.variables) is None
    with pytest.raises(ValueError, match="stranger"):
        m._train_roles([Variable(object(), "stranger")])
    i.trainable = True
    assert m.trainable_variables == m.variables


def test_step_queue_keeps_subset_steps_apart_and_declines_their_censor():
    from openrec_amd.tf2.recommenders._base import _StepQueue
    q = _StepQueue()
    ids = np.arange(4, dtype=np.int32)
    q.add(object(), ("pair", ("user",)), (ids, ids, ids), lambda bufs, K: None, subset=True)
    assert q.subset and not q.mark_censor((ids, ids, ids))
    q2 = _StepQueue()
    q2.add(object(), ("pair", None), (ids, ids, ids), lambda bufs, K: None)
    assert not q2.subset and q2.mark_censor((ids, ids, ids))


# ---- the composed expectation of tests/test_gpu_subset.py against the reference's own class text ---------------------------
def _subset_fixtures():
    from conftest import GOLDEN
    d = os.path.join(GOLDEN, "refstub")
    return sorted(f for f in os.listdir(d) if "sub_" in f and f.endswith(".npz")) if os.path.isdir(d) else []


def test_the_subset_fixtures_are_there():
    names = _subset_fixtures()
    assert 6 <= len(names) <= 10 and {n.split("sub_")[0] for n in names} == {"bpr", "ucml", "wrmf"}


@pytest.mark.parametrize("dtype,tol", [(np.float64, 2e-7), (np.float32, 1e-5)])
@pytest.mark.parametrize("fname", _subset_fixtures())
def test_composed_expectation_matches_the_reference_text(fname, dtype, tol):
    """tests/golden/make_golden_subset.py ran the reference's BPR / UCML / WRMF with apply_gradients on a subset of the
    variables; subset_expect.expect_step (the oracle's gradients, then `apply` for the trained roles only) must give the same
    losses -- l2 over the frozen rows included --, trained tables and slots, and leave the same tables alone.  Bounds as
    tests/test_reference_goldens.py: 2e-7 in float64 (the files store float32), 1e-5 in float32."""
    from conftest import GOLDEN, OPT_KW, rel_err
    from oracle import numpy_oracle as orc
    from subset_expect import expect_step
    g = dict(np.load(os.path.join(GOLDEN, "refstub", fname)))
    model, roles, _, optkind, _ = fname[:-4].split("_")
    model = model[:-3]
    names = {"u": ("user", "U"), "i": ("item", "V"), "b": ("bias", "b")}
    train = tuple(names[r][0] for r in roles)
    W = {k: g["in_" + k].astype(dtype) for k in ("U", "V", "b")}
    kw = OPT_KW[optkind]
    oo = {"sgd": orc.SGD, "adagrad": orc.Adagrad, "adam": orc.AdamTFSparse}[optkind](**kw)
    losses = []
    for s in range(int(g["steps"])):
        uid, pid = np.roll(g["in_uid"], s), np.roll(g["in_pid"], 2 * s)
        third = np.roll(g["in_label"], s).astype(dtype) if model == "wrmf" else np.roll(g["in_nid"], 3 * s)
        losses.append(expect_step(model, W["U"], W["V"], W["b"], (uid, pid, third), oo, train))
    assert rel_err(np.array(losses, np.float64), g["losses"]) < tol
    trained = {names[r][1] for r in roles}
    slots = {"sgd": {}, "adagrad": {"acc": getattr(oo, "acc", None)}, "adam": {"m": getattr(oo, "m", None), "v": getattr(oo, "v", None)}}[optkind]
    for k in ("U", "V", "b"):
        if k in trained:
            assert rel_err(W[k], g["out_" + k]) < tol, k
            for short, store in slots.items():
                assert rel_err(store[k], g["slot_%s_%s" % (k, short)]) < tol, (k, short)
        else:
            assert np.array_equal(g["out_" + k], g["in_" + k]) and np.array_equal(W[k].astype(np.float32), g["in_" + k]), k
            assert not any(key.startswith("slot_%s_" % k) for key in g), k
