"""CPU: the two float64 references of the VBPR step agree (tests/vbpr_ref.py), a float32 evaluation of the step has the headroom the
GPU tests rely on -- inside both worst-case bounds and inside conftest.delta_check on U, V, b and E --, the launch geometry, and the
argument checks of rt.VBPR, rt.ItemFeatures and the tf2 class that need no device."""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest

import vbpr_cases as vc
import vbpr_ref as vr
from conftest import delta_check


def _f64(d):
    return {k: (v.astype(np.float64) if v is not None and v.dtype == np.float32 else v) for k, v in d.items()}


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = float(np.abs(a - b).max())
    assert err <= 1e-12 * max(1.0, float(np.abs(b).max())), (what, err)


def _inside(err, bound, what):
    """err <= bound element by element (a bound of 0 -- a pair with p == n -- asks for an exact 0)"""
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"{what}: worst error {ratio:.3g} of the bound")
    assert (err <= bound).all(), (what, ratio)


# ---- the hand-written formulas against autograd of the score written directly -------------------------------------------------------
@pytest.mark.parametrize("weights,bias,l2_reg,l2_proj", list(itertools.product((False, True), (False, True), (0.0, 0.01), (0.0, 0.001))))
def test_the_two_references_agree(weights, bias, l2_reg, l2_proj):
    c = _f64(vc.make(dict(vc.GENERAL, bias=bias, weights=weights, seed=11)))
    args = (c["U"], c["V"], c["b"], c["E"], c["F"], c["uid"][0], c["pid"][0], c["nid"][0], None if c["w"] is None else c["w"][0])
    a = vr.grads(*args, l2_reg=l2_reg, l2_proj=l2_proj)
    t = vr.torch_grads(*args, l2_reg=l2_reg, l2_proj=l2_proj)
    GU, GV, Gb = vr.dense(a, (c["U"].shape, c["V"].shape), c["uid"][0], c["pid"][0], c["nid"][0])
    _close(a["loss"], t["loss"], "loss"); _close(a["l2"], t["l2"], "l2")
    _close(GU, t["GU"], "user"); _close(GV, t["GV"], "item"); _close(a["dE"], t["dE"], "proj")
    if bias:
        _close(Gb, t["Gb"], "bias")
    assert np.abs(a["dE"]).max() > 0 and np.abs(GU[:, c["V"].shape[1]:]).max() > 0          # (the content half is alive)


def test_the_clamp_and_a_zero_weight():
    """x below -30 has no loss gradient; a weight of 0 leaves a triplet its l2 part"""
    c = _f64(vc.make(dict(vc.GENERAL, bias=True, weights=True, seed=12), scale=3.0))
    args = (c["U"], c["V"], c["b"], c["E"], c["F"], c["uid"][0], c["pid"][0], c["nid"][0], c["w"][0])
    a = vr.grads(*args, l2_reg=0.5)
    assert (a["x"] < -30).any()
    dead = (a["x"] < -30) | (c["w"][0] == 0)
    assert np.array_equal(a["gbp"][dead], np.zeros(dead.sum())) and np.abs(a["gbp"][~dead]).max() > 0
    assert np.allclose(a["gp"][dead], 0.5 * c["V"][c["pid"][0]][dead])
    t = vr.torch_grads(*args, l2_reg=0.5)
    _close(vr.dense(a, (c["U"].shape, c["V"].shape), c["uid"][0], c["pid"][0], c["nid"][0])[1], t["GV"], "item")


# ---- float32 headroom: what the device is asked for, NumPy float32 delivers ----------------------------------------------------------
@pytest.mark.parametrize("seed", range(20))
def test_float32_evaluation_stays_inside_the_bounds(seed):
    case = dict(vc.GENERAL, bias=True, weights=False, seed=500 + seed)
    c32 = vc.make(case)
    c64 = _f64(c32)
    ids = (c32["uid"][0], c32["pid"][0], c32["nid"][0])
    g32 = vr.grads(c32["U"], c32["V"], c32["b"], c32["E"], c32["F"], *ids, l2_reg=vc.L2_REG, l2_proj=vc.L2_PROJ)
    g64 = vr.grads(c64["U"], c64["V"], c64["b"], c64["E"], c64["F"], *ids, l2_reg=vc.L2_REG, l2_proj=vc.L2_PROJ)
    # the projection
    pb = vr.proj_bound(c32["F"], c32["E"], ids[1], ids[2])
    _inside(np.abs(g32["delta"].astype(np.float64) - vr.project(c32["F"], c32["E"], ids[1], ids[2])), pb, "projection")
    # dE, against three chunks of 64
    db = vr.dproj_bound(g64["df"], g64["R"], 64, 3)
    _inside(np.abs(g32["dE"].astype(np.float64) - vc.L2_PROJ * c64["E"] - g64["df"].T @ g64["R"]), db, "dE")
    # the step
    t32 = {k: c32[k].copy() for k in ("U", "V", "b", "E")}
    t64 = {k: c64[k].copy() for k in ("U", "V", "b", "E")}
    vr.step(t32["U"], t32["V"], t32["b"], t32["E"], c32["F"], *ids, vr.make_opt("sgd"), l2_reg=vc.L2_REG, l2_proj=vc.L2_PROJ)
    vr.step(t64["U"], t64["V"], t64["b"], t64["E"], c64["F"], *ids, vr.make_opt("sgd"), l2_reg=vc.L2_REG, l2_proj=vc.L2_PROJ)
    for k in ("U", "V", "b", "E"):
        delta_check(c32[k], t32[k], t64[k].astype(np.float32), steps=1, what=f"seed {seed} {k}")


def test_train_mask_of_the_reference_leaves_the_other_tables():
    c = _f64(vc.make(dict(vc.GENERAL, bias=True, weights=False, seed=13)))
    for train in (("user",), ("item",), ("bias",), ("proj",), ("user", "proj")):
        t = {k: c[k].copy() for k in ("U", "V", "b", "E")}
        vr.step(t["U"], t["V"], t["b"], t["E"], c["F"], c["uid"][0], c["pid"][0], c["nid"][0], vr.make_opt("adam"), train=train)
        for k, role in (("U", "user"), ("V", "item"), ("b", "bias"), ("E", "proj")):
            assert np.array_equal(t[k], c[k]) == (role not in train), (train, k)


# ---- the launch geometry (host only) --------------------------------------------------------------------------------------------------
def test_geometry():
    from openrec_amd import runtime as rt
    g = rt.vbpr_geometry(192, 50, 20, 64)
    assert g == dict(chunk_rows=64, chunks=3, dim=32, tile_rows=64)
    assert rt.vbpr_geometry(192, 50, 20, 128)["chunks"] == 2
    for B, Fd, Dc in ((192, 50, 20), (65536, 512, 32), (1, 1, 1), (10 ** 6, 8192, 128), (3 * 10 ** 6, 7, 128)):
        g = rt.vbpr_geometry(B, Fd, Dc)
        assert g["chunk_rows"] % 64 == 0 and g["chunk_rows"] >= 64 and g["dim"] % 16 == 0 and g["dim"] >= Dc
        assert (g["chunks"] - 1) * g["chunk_rows"] < B <= g["chunks"] * g["chunk_rows"] and g["chunks"] <= 65535
    for bad in (dict(batch_chunk=96), dict(batch_chunk=-64), dict(Dc=0), dict(Dc=129), dict(Fd=0), dict(Fd=8193), dict(B=2 ** 31 - 256)):
        kw = dict(dict(B=192, Fd=50, Dc=20, batch_chunk=0), **bad)
        with pytest.raises(ValueError):
            rt.vbpr_geometry(kw["B"], kw["Fd"], kw["Dc"], kw["batch_chunk"])


# ---- argument checks that need no device ----------------------------------------------------------------------------------------------
def _fake_table(ctx, rows, dim):
    return SimpleNamespace(ctx=ctx, rows=rows, dim=dim, shape=(rows, dim))


def _fake_features(rt, ctx, rows, dim):
    f = object.__new__(rt.ItemFeatures)
    f.ctx, f.rows, f.dim = ctx, rows, dim
    return f


def test_item_features_refuses_what_it_cannot_hold():
    from openrec_amd import runtime as rt
    for bad in (np.zeros((4, 3), np.float64), np.zeros(12, np.float32), np.zeros((4, 6), np.float32)[:, ::2], np.zeros((4, 0), np.float32),
                np.zeros((0, 3), np.float32), np.zeros((2, 8193), np.float32)):
        with pytest.raises(ValueError, match="ItemFeatures"):
            rt.ItemFeatures(bad)


def test_vbpr_refuses_mismatched_tables():
    from openrec_amd import runtime as rt
    ctx, other = object(), object()
    T = lambda r, d, c=ctx: _fake_table(c, r, d)
    ok = dict(U=T(30, 32), V=T(40, 12), b=T(40, 1), E=T(50, 20), features=_fake_features(rt, ctx, 40, 50))
    rt.VBPR(**ok)
    for what, bad in (("user dim", dict(U=T(30, 33))), ("feature rows", dict(features=_fake_features(rt, ctx, 41, 50))),
                      ("rows for features", dict(E=T(51, 20))), ("bias must be", dict(b=T(40, 2))), ("bias must be", dict(b=T(39, 1))),
                      ("Dc", dict(E=T(50, 0), U=T(30, 12))), ("above 128", dict(E=T(50, 129), U=T(30, 141))),
                      ("above 256", dict(U=T(30, 257), V=T(40, 200), E=T(50, 57))), ("contexts", dict(V=T(40, 12, other))),
                      ("ItemFeatures", dict(features=np.zeros((40, 50), np.float32)))):
        with pytest.raises(ValueError, match=what):
            rt.VBPR(**dict(ok, **bad))
    net = rt.VBPR(**ok)
    ids = np.zeros(8, np.int32)
    with pytest.raises(ValueError, match="unknown table"):
        net.step(None, ids, ids, ids, train=("projection",))
    with pytest.raises(ValueError, match="batch_chunk"):
        net.step(None, ids, ids, ids, batch_chunk=96)
    with pytest.raises(ValueError, match="l2_proj"):
        net.step(None, ids, ids, ids, l2_proj=-1.0)
    with pytest.raises(ValueError, match="l2_reg"):
        net.step(None, ids, ids, ids, l2_reg=float("nan"))
    with pytest.raises(ValueError, match='"bias" named'):
        rt.VBPR(**dict(ok, b=None)).step(None, ids, ids, ids, train=("bias",))


def test_tf2_class_refuses_bad_dims_before_any_device_work():
    from openrec_amd.tf2.recommenders import VBPR
    F = np.zeros((40, 50), np.float32)
    for kw in (dict(dim_user_embed=32, dim_item_embed=32), dict(dim_user_embed=32, dim_item_embed=0), dict(dim_user_embed=200, dim_item_embed=60),
               dict(dim_user_embed=300, dim_item_embed=200), dict(dim_user_embed=32, dim_item_embed=12, total_items=41),
               dict(dim_user_embed=32, dim_item_embed=12, l2_reg=-1.0), dict(dim_user_embed=32, dim_item_embed=12, l2_reg_mlp=float("inf"))):
        with pytest.raises(ValueError):
            VBPR(**dict(dict(total_users=30, total_items=40, item_features=F), **kw))
