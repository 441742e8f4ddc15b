"""Top-K recommendation on the device (orx_recommend_topk / orx_topk_rows, rt.recommend_topk / rt.topk_rows,
Recommender.recommend, tf.math.top_k of the shim) against a NumPy selection over the scorer's own scores: a sort by
(-score, item id) of `rt.score_all_items` of the same tables, excluded and NaN items removed, padded with -1 / -inf.
Item ids and score bits must be EQUAL."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KINDS = ("dot", "l2", "gmf")


def _rt():
    from openrec_amd import runtime as rt
    return rt


def expect_topk(S, k, excl=None):
    """the selection in NumPy: per row the k best non-NaN, non-excluded scores, (score desc, id asc), padded"""
    S = np.asarray(S, np.float32)
    n, m = S.shape
    items = np.full((n, k), -1, np.int32)
    vals = np.full((n, k), -np.inf, np.float32)
    for q in range(n):
        s = S[q]
        ok = ~np.isnan(s)
        if excl is not None and len(excl[q]):
            ok[np.asarray(excl[q], np.int64)] = False
        idx = np.nonzero(ok)[0]
        sv = s[idx]
        if idx.size > k:                       # (every item tied with the k-th stays a candidate)
            kth = np.partition(sv, idx.size - k)[idx.size - k]
            keep = sv >= kth
            idx, sv = idx[keep], sv[keep]
        order = np.lexsort((idx, -sv))[:k]
        items[q, :order.size] = idx[order]
        vals[q, :order.size] = sv[order]
    return items, vals


def assert_same(got, want, what=""):
    gi, gs = (np.asarray(x) for x in got)
    wi, ws = want
    assert gi.shape == wi.shape and gs.shape == ws.shape, what
    bad = np.nonzero((gi != wi).any(axis=1) | (gs.view(np.int32) != ws.view(np.int32)).any(axis=1))[0]
    assert bad.size == 0, f"{what}: rows {bad[:5]} differ, e.g. got {gi[bad[0], :8]} / {gs[bad[0], :8]}, " \
                          f"want {wi[bad[0], :8]} / {ws[bad[0], :8]}"


def tables(rt, NU, NI, D, bias=True, seed=0, ctx=None):
    rng = np.random.default_rng(seed)
    U = rt.Table(NU, D, ctx); U.write(rng.standard_normal((NU, D)).astype(np.float32) * 0.3)
    V = rt.Table(NI, D, ctx); V.write(rng.standard_normal((NI, D)).astype(np.float32) * 0.3)
    b = None
    if bias:
        b = rt.Table(NI, 1, ctx); b.write(rng.standard_normal((NI, 1)).astype(np.float32))
    w = rt.Table(D, 1, ctx); w.write(rng.uniform(0.5, 1.5, (D, 1)).astype(np.float32))
    return U, V, b, w


def random_excl(rng, n, NI, max_len=300):
    rows = [rng.choice(NI, int(rng.integers(0, max_len)), replace=False) for _ in range(n)]
    rows[0] = np.zeros(0, np.int64)            # an empty list
    return rows


# ---- 1. every kind, with and without bias, every tile width and the non-MFMA route -------------------------------
@pytest.mark.parametrize("D", [16, 50, 64, 128, 200, 300])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_every_kind_matches_the_scorer(kind, bias, D):
    rt = _rt()
    NU, NI, n = 500, 100003, 300
    U, V, b, w = tables(rt, NU, NI, D, bias, seed=D)
    rng = np.random.default_rng(D + 7)
    uid = rng.integers(0, NU, n).astype(np.int32)
    rows = random_excl(rng, n, NI)
    mask = rt.SparseMask.from_lists(rows, NI)
    S = rt.score_all_items(kind, U, V, b, uid, w=w)
    want_i, want_s = expect_topk(S, 1024, rows)
    for k in (1, 10, 100, 1024):
        got = rt.recommend_topk(kind, U, V, b, uid, k, excl=mask, w=w)
        assert_same(got, (want_i[:, :k], want_s[:, :k]), f"{kind} bias={bias} D={D} k={k}")


# ---- 2. ties and the overflow fallback ------------------------------------------------------------------------------
def test_repeated_item_rows_tie_by_id():
    rt = _rt()
    NU, NI, D, n = 200, 100003, 64, 100
    rng = np.random.default_rng(3)
    U = rt.Table(NU, D); U.write(rng.standard_normal((NU, D)).astype(np.float32))
    base = rng.standard_normal((40, D)).astype(np.float32)
    V = rt.Table(NI, D); V.write(base[rng.integers(0, 40, NI)])
    b = rt.Table(NI, 1); b.write(np.zeros((NI, 1), np.float32))
    uid = rng.integers(0, NU, n).astype(np.int32)
    rows = random_excl(rng, n, NI, 50)
    S = rt.score_all_items("dot", U, V, b, uid)
    want = expect_topk(S, 1024, rows)
    for k in (10, 100, 1024):
        got = rt.recommend_topk("dot", U, V, b, uid, k, excl=rt.SparseMask.from_lists(rows, NI))
        assert_same(got, (want[0][:, :k], want[1][:, :k]), f"k={k}")
        assert (np.diff(got[0][:, :k], axis=1)[np.diff(got[1][:, :k], axis=1) == 0] > 0).all()


@pytest.mark.parametrize("kind", KINDS)
def test_a_constant_table_takes_the_fallback_and_stays_exact(kind):
    rt = _rt()
    NU, NI, D, n = 50, 100003, 32, 40
    U = rt.Table(NU, D); U.fill(0.25)
    V = rt.Table(NI, D); V.fill(0.5)
    b = rt.Table(NI, 1); b.fill(0.125)
    w = rt.Table(D, 1); w.fill(1.0)
    rng = np.random.default_rng(4)
    uid = rng.integers(0, NU, n).astype(np.int32)
    rows = random_excl(rng, n, NI, 30)
    S = rt.score_all_items(kind, U, V, b, uid, w=w)
    assert (S == S[0, 0]).all()
    for k in (1, 100, 1024):
        got = rt.recommend_topk(kind, U, V, b, uid, k, excl=rt.SparseMask.from_lists(rows, NI), w=w)
        assert_same(got, expect_topk(S, k, rows), f"{kind} k={k}")


# ---- 3. edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NI", [500, 20000])
def test_padding_nan_and_minus_inf(NI):
    """fewer eligible items than k, every item excluded, k > items (500 items), a NaN item row and a -inf bias"""
    rt = _rt()
    NU, D, n = 30, 64, 6
    rng = np.random.default_rng(NI)
    U, V, b, w = tables(rt, NU, NI, D, True, seed=11)
    Vh = V.read(); Vh[7] = np.nan; V.write(Vh)
    bh = b.read(); bh[11] = -np.inf; b.write(bh)
    uid = np.arange(n, dtype=np.int32)
    rows = [np.zeros(0, np.int64), np.setdiff1d(np.arange(NI), [1, 5, 7, 11, 300]), np.arange(NI),
            rng.choice(NI, 40, replace=False), np.zeros(0, np.int64), np.arange(0, NI, 2)]
    mask = rt.SparseMask.from_lists(rows, NI)
    for kind in KINDS:
        S = rt.score_all_items(kind, U, V, b, uid, w=w)
        assert np.isnan(S[:, 7]).all() and (S[:, 11] == -np.inf).all()
        for k in (10, 1024):
            got = rt.recommend_topk(kind, U, V, b, uid, k, excl=mask, w=w)
            assert_same(got, expect_topk(S, k, rows), f"{kind} NI={NI} k={k}")
            assert not (got[0] == 7).any()
            assert (got[0][2] == -1).all() and (got[1][2] == -np.inf).all()
            assert list(got[0][1][:4]) == sorted(set([1, 5, 300]), key=lambda j: (-S[1, j], j)) + [11]
        if NI < 1024:
            assert (got[0][0] == 11).sum() == 1 and got[0][0][NI - 2] == 11 and (got[0][0][NI - 1:] == -1).all()


def test_argument_errors():
    rt = _rt()
    U, V, b, w = tables(rt, 10, 1000, 16, True)
    uid = np.arange(3, dtype=np.int32)
    for k in (0, 1025):
        with pytest.raises(ValueError, match="k"):
            rt.recommend_topk("dot", U, V, b, uid, k)
    lib = U.ctx._lib
    from openrec_amd import _ffi
    oi = np.empty((3, 5), np.int32); os_ = np.empty((3, 5), np.float32)
    rc = lib.orx_recommend_topk(U.ctx._h, 0, U._h, V._h, b._h, None, uid.ctypes.data, 3, None, None, 1025, 0,
                                oi.ctypes.data, os_.ctypes.data)
    assert rc == _ffi.ORX_ERR_ARG and b"k" in lib.orx_last_error()
    with pytest.raises(IndexError):
        rt.recommend_topk("dot", U, V, b, np.array([0, 10], np.int32), 5)
    with pytest.raises(IndexError):
        rt.recommend_topk("dot", U, V, b, np.array([0, -1], np.int32), 5)
    bad = rt.SparseMask(np.array([0, 1, 1, 2], np.int64), np.array([3, 1000], np.int32), 1000)
    with pytest.raises(IndexError):
        rt.recommend_topk("dot", U, V, b, uid, 5, excl=bad)
    with pytest.raises(IndexError):
        rt.topk_rows(np.zeros((3, 1000), np.float32), 5, excl=bad)
    got = rt.recommend_topk("dot", U, V, b, uid, 5)               # the context is usable afterwards
    assert_same(got, expect_topk(rt.score_all_items("dot", U, V, b, uid), 5))


# ---- 4. full size --------------------------------------------------------------------------------------------------------
def expect_topk_device(ds, k):
    """expect_topk for a DeviceScores without NaN or exclusions: the k-th value per row on the device, the candidates
    (everything tied with it included) on the host"""
    import torch
    t = ds.tensor
    kth = torch.topk(t, k, dim=1).values[:, -1:]
    r, c = torch.nonzero(t >= kth, as_tuple=True)
    vals = t[r, c].cpu().numpy(); r = r.cpu().numpy(); c = c.cpu().numpy()
    n = t.shape[0]
    items = np.empty((n, k), np.int32); scores = np.empty((n, k), np.float32)
    order = np.lexsort((c, -vals, r))
    start = np.searchsorted(r[order], np.arange(n))
    for q in range(n):
        o = order[start[q]:start[q] + k]
        items[q], scores[q] = c[o], vals[o]
    return items, scores


@pytest.mark.parametrize("kind", KINDS)
def test_full_size_1000_users_1m_items(kind):
    rt = _rt()
    NU, NI, D, n, k = 20000, 1 << 20, 64, 1000, 100
    U = rt.Table(NU, D); U.init_uniform(-0.5, 0.5, seed=1)
    V = rt.Table(NI, D); V.init_uniform(-0.5, 0.5, seed=2)
    b = rt.Table(NI, 1); b.init_uniform(-0.1, 0.1, seed=3)
    w = rt.Table(D, 1); w.init_uniform(0.5, 1.5, seed=4)
    uid = np.random.default_rng(5).integers(0, NU, n).astype(np.int32)
    want = expect_topk_device(rt.score_all_items(kind, U, V, b, uid, w=w, device=True), k)
    got = rt.recommend_topk(kind, U, V, b, uid, k, w=w)
    assert_same(got, want, kind)
    again = rt.recommend_topk(kind, U, V, b, uid, k, w=w)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1].view(np.int32), got[1].view(np.int32))
    dev = rt.recommend_topk(kind, U, V, b, uid, k, w=w, device=True)
    assert_same((dev[0].cpu().numpy(), dev[1].cpu().numpy()), want, kind + " device outputs")


# ---- 5. no materialisation: 100 000 users x 1 M items (400 GB of scores) -----------------------------------------------
def test_100k_users_1m_items():
    rt = _rt()
    NU, NI, D, n, k = 100000, 1 << 20, 64, 100000, 10
    U = rt.Table(NU, D); U.init_uniform(-0.5, 0.5, seed=6)
    V = rt.Table(NI, D); V.init_uniform(-0.5, 0.5, seed=7)
    b = rt.Table(NI, 1); b.init_uniform(-0.1, 0.1, seed=8)
    uid = np.arange(n, dtype=np.int32)
    got = rt.recommend_topk("dot", U, V, b, uid, k)
    assert got[0].shape == (n, k) and (got[0] >= 0).all()
    sample = np.random.default_rng(9).choice(n, 64, replace=False)
    want = expect_topk_device(rt.score_all_items("dot", U, V, b, uid[sample], device=True), k)
    assert_same((got[0][sample], got[1][sample]), want, "sampled users")


# ---- 6. orx_topk_rows --------------------------------------------------------------------------------------------------
def test_topk_rows_on_device_scores_and_host_arrays():
    rt = _rt()
    NU, NI, D, n = 100, 30011, 64, 70
    U, V, b, w = tables(rt, NU, NI, D, True, seed=21)
    rng = np.random.default_rng(22)
    uid = rng.integers(0, NU, n).astype(np.int32)
    rows = random_excl(rng, n, NI)
    mask = rt.SparseMask.from_lists(rows, NI)
    ds = rt.score_all_items("l2", U, V, b, uid, device=True)
    S = np.array(ds.tensor.cpu().numpy())
    S[3, ::7] = np.nan
    S[4, :] = 1.5                                               # all tied
    for k in (1, 37, 1024):
        want = expect_topk(S, k, rows)
        assert_same(rt.topk_rows(S, k, excl=mask), want, f"host k={k}")
        assert_same(rt.topk_rows(S, k, excl=mask._dense()), want, f"host dense mask k={k}")
        assert_same(rt.topk_rows(ds, k), expect_topk(np.asarray(ds.tensor.cpu()), k), f"device k={k}")
        assert_same(rt.topk_rows(ds, k, excl=mask), expect_topk(np.asarray(ds.tensor.cpu()), k, rows), f"device excl k={k}")


# ---- 7. the model level -------------------------------------------------------------------------------------------------
def _dataset(NU, NI, n_rec, seed):
    from openrec_amd.tf2.data import Dataset
    rng = np.random.default_rng(seed)
    raw = np.zeros(n_rec, dtype=[("user_id", np.int32), ("item_id", np.int32)])
    raw["user_id"], raw["item_id"] = rng.integers(0, NU, n_rec), rng.integers(0, NI, n_rec)
    return Dataset(raw, NU, NI, seed=seed)


@pytest.mark.parametrize("name", ["bpr", "bpr_nobias", "ucml", "gmf", "wrmf"])
def test_recommend_after_adam_steps(name):
    from openrec_amd.tf2 import compat
    compat.install()
    import tensorflow as tf
    from openrec_amd.tf2.recommenders import BPR, GMF, UCML, WRMF
    rt = _rt()
    NU, NI, D, B = 600, 5000, 32, 256
    model = {"bpr": lambda: BPR(D, D, NU, NI), "bpr_nobias": lambda: BPR(D, D, NU, NI, use_item_bias=False),
             "ucml": lambda: UCML(D, D, NU, NI), "gmf": lambda: GMF(D, D, NU, NI), "wrmf": lambda: WRMF(D, D, NU, NI)}[name]()
    opt = tf.keras.optimizers.Adam(0.01)
    rng = np.random.default_rng(31)
    for _ in range(5):
        u = rng.integers(0, NU, B).astype(np.int32)
        with tf.GradientTape() as tape:
            if name in ("gmf", "wrmf"):
                loss = model(u, rng.integers(0, NI, B).astype(np.int32), rng.integers(0, 2, B).astype(np.float32))
            else:
                loss = model(u, rng.integers(0, NI, B).astype(np.int32), rng.integers(0, NI, B).astype(np.int32))
        grads = tape.gradient(loss, model.trainable_variables)
        opt.apply_gradients(zip(grads, model.trainable_variables))
    train, val = _dataset(NU, NI, 20000, 1), _dataset(NU, NI, 3000, 2)
    batch = next(iter(val.evaluation(batch_size=64, excl_datasets=[train])))
    uid, excl = batch["user_id"], batch["excl_mask"]
    items, scores = model.recommend(uid, 50, excl)
    U, V, b = model._tables()
    kind = model._score_kind
    w = model.mlp.layers[0].kernel if kind == "gmf" else None
    assert_same((items, scores), rt.recommend_topk(kind, U, V, b, uid, 50, excl=excl, w=w), name)
    S = rt.score_all_items(kind, U, V, b, uid, w=w)
    assert_same((items, scores), expect_topk(S, 50, [excl.row(q) for q in range(len(uid))]), name + " vs the scorer")
    # the TF 2.0 idiom on the reference API: tf.math.top_k(model.inference(uid), k), no exclusion
    values, indices = tf.math.top_k(model.inference(uid), k=20)
    want_i, want_s = expect_topk(S, 20)
    assert np.array_equal(np.asarray(indices), want_i) and np.array_equal(np.asarray(values).view(np.int32), want_s.view(np.int32))
    v1, i1 = tf.nn.top_k(np.asarray(S[0]), 5)
    assert np.array_equal(np.asarray(i1), want_i[0, :5]) and np.array_equal(np.asarray(v1), want_s[0, :5])
