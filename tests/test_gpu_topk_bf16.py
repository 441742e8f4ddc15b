"""recommend_topk(prefilter="bf16"): the bf16 matrix-core prefilter must return, bit for bit, the NumPy selection over
`rt.score_all_items` (the reference of test_gpu_topk.py), and must really have run: every comparison also checks the route
through Context.stat, since a silent fall-back to the fp32 route would pass every equality.  20 003 items: no multiple of a
tile or chunk, and more than the threshold sample of 8 192 for every k used."""
import numpy as np
import pytest

from test_gpu_topk import KINDS, assert_same, expect_topk, random_excl, tables

pytestmark = pytest.mark.gpu

NI = 20003


def _rt():
    from openrec_amd import runtime as rt
    return rt


def check(rt, kind, U, V, b, w, uid, rows, ks, dense, what):
    """prefiltered top-k against the reference for every k; `dense`: how many users must have taken the dense fallback"""
    S = rt.score_all_items(kind, U, V, b, uid, w=w)
    want = expect_topk(S, max(ks), rows)
    mask = rt.SparseMask.from_lists(rows, NI) if rows is not None else None
    for k in ks:
        got = rt.recommend_topk(kind, U, V, b, uid, k, excl=mask, w=w, prefilter="bf16")
        assert_same(got, (want[0][:, :k], want[1][:, :k]), f"{what} k={k}")
        st = {s: U.ctx.stat(s) for s in ("topk_prefiltered", "topk_dense", "topk_candidates")}
        print(what, "k =", k, st)
        assert st["topk_dense"] == dense and st["topk_prefiltered"] == len(uid) - dense, f"{what} k={k}: {st}"


@pytest.mark.parametrize("D", [16, 50, 64, 200])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_every_kind_and_width(kind, bias, D):
    rt = _rt()
    U, V, b, w = tables(rt, 400, NI, D, bias, seed=D)
    rng = np.random.default_rng(D + 7)
    for n in (70, 300):                    # a partial user tile; several user tiles of the widest form
        uid = rng.integers(0, 400, n).astype(np.int32)
        check(rt, kind, U, V, b, w, uid, random_excl(rng, n, NI), (1, 10, 100, 1024), 0, f"{kind} bias={bias} D={D} n={n}")


@pytest.mark.parametrize("kind", ["dot", "l2"])
def test_clustered_rows_need_the_margin(kind):
    """every item row is one of 40 base rows times (1 + d), |d| <= 2^-9: the bf16 copies of a cluster coincide, and a filter
    without the margin loses between 29 and 816 of the 70 users' winners here (a NumPy emulation of the bf16 pass)"""
    rt = _rt()
    rng = np.random.default_rng(5)
    D, n = 64, 70
    U = rt.Table(200, D); U.write(rng.standard_normal((200, D)).astype(np.float32))
    base = rng.standard_normal((40, D)).astype(np.float32)
    V = rt.Table(NI, D)
    V.write(base[rng.integers(0, 40, NI)] * (1.0 + rng.uniform(-2.0 ** -9, 2.0 ** -9, (NI, 1))).astype(np.float32))
    uid = rng.integers(0, 200, n).astype(np.int32)
    check(rt, kind, U, V, None, None, uid, None, (10, 100), 0, f"clustered {kind}")


@pytest.mark.parametrize("kind", KINDS)
def test_a_constant_table_overflows_and_stays_exact(kind):
    rt = _rt()
    D, n = 32, 40
    U = rt.Table(50, D); U.fill(0.25)
    V = rt.Table(NI, D); V.fill(0.5)
    b = rt.Table(NI, 1); b.fill(0.125)
    w = rt.Table(D, 1); w.fill(1.0)
    rng = np.random.default_rng(4)
    uid = rng.integers(0, 50, n).astype(np.int32)
    check(rt, kind, U, V, b, w, uid, random_excl(rng, n, NI, 30), (1, 100), n, f"constant {kind}")


@pytest.mark.parametrize("kind", KINDS)
def test_non_finite_values(kind):
    """a NaN item row, a +inf item row, a -inf bias, a user row with a NaN: nothing lost, nothing returned that the fp32 route skips"""
    rt = _rt()
    U, V, b, w = tables(rt, 30, NI, 64, True, seed=11)
    Vh = V.read(); Vh[7, 3] = np.nan; Vh[9000, 5] = np.inf; V.write(Vh)
    bh = b.read(); bh[11] = -np.inf; b.write(bh)
    Uh = U.read(); Uh[4, 2] = np.nan; U.write(Uh)
    uid = np.arange(12, dtype=np.int32)
    S = rt.score_all_items(kind, U, V, b, uid, w=w)
    assert np.isnan(S[:, 7]).all() and np.isnan(S[4]).all() and np.isinf(S[0, 9000]) and (S[0, 11] == -np.inf)
    for k in (10, 1024):
        got = rt.recommend_topk(kind, U, V, b, uid, k, w=w, prefilter="bf16")
        assert_same(got, expect_topk(S, k), f"{kind} k={k}")
        assert U.ctx.stat("topk_prefiltered") == 11 and U.ctx.stat("topk_dense") == 1      # (the NaN user: no threshold)
        assert not (got[0] == 7).any() and (got[0][4] == -1).all()


def test_outside_the_route_and_arguments():
    rt = _rt()
    rng = np.random.default_rng(2)
    uid = rng.integers(0, 100, 70).astype(np.int32)
    U, V, b, w = tables(rt, 100, NI, 300, True, seed=1)
    S = rt.score_all_items("dot", U, V, b, uid)
    assert_same(rt.recommend_topk("dot", U, V, b, uid, 10, prefilter="bf16"), expect_topk(S, 10), "D=300")
    assert U.ctx.stat("topk_prefiltered") == 0 and U.ctx.stat("topk_dense") == 70
    assert rt.topk_geometry("dot", 70, NI, 300, 10, prefilter="bf16")["route"] == 0
    g = rt.topk_geometry("l2", 70, NI, 64, 10, prefilter="bf16")
    assert g["route"] == 2 and g["sample"] == 8192 and g["copy_bytes"] == 20032 * 64 * 2 + 20032 * 8 and g["user_tile"] == 128
    assert rt.topk_geometry("l2", 70, NI, 64, 10)["route"] == 0 and rt.topk_geometry("dot", 70, NI, 64, 10)["route"] == 1
    with pytest.raises(ValueError):
        rt.recommend_topk("dot", U, V, b, uid, 10, prefilter="fp16")
    U, V, b, w = tables(rt, 100, NI, 64, True, seed=1)
    host = rt.recommend_topk("gmf", U, V, b, uid, 100, w=w, prefilter="bf16")
    dev = rt.recommend_topk("gmf", U, V, b, uid, 100, w=w, prefilter="bf16", device=True)
    assert U.ctx.stat("topk_prefiltered") == 70
    assert_same((dev[0].cpu().numpy(), dev[1].cpu().numpy()), host, "device outputs")
