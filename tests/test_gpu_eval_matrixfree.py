"""Ranking metrics without a score matrix (orx_rank_metrics_matrixfree, rt.rank_metrics_matrixfree,
Recommender.evaluate(score_matrix=False)) against the materialised path `rt.rank_metrics_csr(kind=...)` on the same tables:
AUC, NDCG and Recall must be EQUAL bit for bit (NaN-aware).  Both paths count the same integers from bit-identical scores and
add them up in the same fixed order, so no tolerance applies.  One case per kind is also held to oracle/metrics_oracle.py on
`rt.score_all_items` scores with the tolerances of tests/test_metrics.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

AT = [1, 10, 100]
POS_COUNTS = (0, 1, 7, 8, 15, 16, 63, 64, 150)     # cross every STEPS form (7 / 15 / 63 thresholds) and span several chunks


def _rt():
    from openrec_amd import runtime as rt
    return rt


def tables(rt, NU, NI, D, bias=True, seed=0, scale=0.3):
    rng = np.random.default_rng(seed)
    U = rt.Table(NU, D); U.write(rng.standard_normal((NU, D)).astype(np.float32) * scale)
    V = rt.Table(NI, D); V.write(rng.standard_normal((NI, D)).astype(np.float32) * scale)
    b = None
    if bias:
        b = rt.Table(NI, 1); b.write(rng.standard_normal((NI, 1)).astype(np.float32) * scale / 0.3)
    w = rt.Table(D, 1); w.write(rng.uniform(0.5, 1.5, (D, 1)).astype(np.float32))
    return U, V, b, w


def make_lists(rng, n, NI, max_pos, full_excl=True):
    """positives / exclusions per user: every count of POS_COUNTS that fits, a positive that is the last item, a positive
    that is also excluded, a user whose exclusions are everything but the positives, a user with empty lists"""
    counts = [c for c in POS_COUNTS if c <= max_pos and c <= NI // 2]
    pos, excl = [], []
    for q in range(n):
        c = counts[(q + 1) % len(counts)]
        p = rng.choice(NI, c, replace=False)
        e = rng.choice(NI, int(rng.integers(0, min(NI, 200))), replace=False)
        if q % 5 != 2:
            e = np.setdiff1d(e, p)                           # (every fifth user keeps the overlap)
        pos.append(p); excl.append(e)
    pos[0] = np.zeros(0, np.int64); excl[0] = np.zeros(0, np.int64)
    if n > 1:
        pos[1] = np.union1d(pos[1], [NI - 1])[-max(1, min(max_pos, len(pos[1]) + 1)):]
        excl[1] = np.setdiff1d(excl[1], [NI - 1])
    if n > 2:
        pos[2] = np.union1d(pos[2][:max(0, max_pos - 1)], [3]); excl[2] = np.union1d(excl[2], [3, 4])
    if n > 3 and full_excl:
        excl[3] = np.setdiff1d(np.arange(NI), pos[3])        # n_eval = 0
    return pos, excl


def both(rt, pos, excl, NI, kind, U, V, b, w, uid, **kw):
    pm, em = rt.SparseMask.from_lists(pos, NI), rt.SparseMask.from_lists(excl, NI)
    ww = w if kind == "gmf" else None
    want = rt.rank_metrics_csr(pm, em, AT, kind=kind, user=U, item=V, bias=b, w=ww, uid=uid)
    got = rt.rank_metrics_matrixfree(pm, em, AT, kind, U, V, b, uid, w=ww, **kw)
    return got, want


def assert_equal(got, want, what=""):
    for key in ("auc", "ndcg", "recall"):
        g, x = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == x.shape, (what, key)
        if not np.array_equal(g, x, equal_nan=True):
            bad = np.nonzero(~((g == x) | (np.isnan(g) & np.isnan(x))).reshape(g.shape[0], -1).all(axis=1))[0]
            raise AssertionError(f"{what}: {key} differs for users {bad[:8]}: got {g[bad[0]]}, want {x[bad[0]]}")


CASES = [  # kind, bias, NI, n, D, longest positive list
    ("dot", True, 33, 1, 24, 7), ("dot", False, 1000, 37, 18, 15), ("dot", True, 70001, 130, 64, 150),
    ("dot", False, 4099, 130, 24, 7), ("dot", True, 1000, 70, 128, 150), ("dot", False, 4099, 37, 64, 15),
    ("gmf", True, 4099, 70, 64, 150), ("gmf", False, 70001, 130, 128, 150), ("gmf", True, 1000, 70, 18, 15),
    ("gmf", False, 33, 37, 24, 7),
    ("l2", True, 4099, 130, 24, 150), ("l2", False, 1000, 37, 64, 15), ("l2", True, 70001, 70, 128, 7), ("l2", True, 33, 1, 18, 7),
]


@pytest.mark.parametrize("kind,bias,NI,n,D,max_pos", CASES)
def test_equals_the_materialised_path(kind, bias, NI, n, D, max_pos):
    rt = _rt()
    NU = 300
    U, V, b, w = tables(rt, NU, NI, D, bias, seed=NI + D)
    rng = np.random.default_rng(NI + n)
    uid = rng.integers(0, NU, n).astype(np.int32)
    pos, excl = make_lists(rng, n, NI, max_pos, full_excl=NI <= 4099)
    got, want = both(rt, pos, excl, NI, kind, U, V, b, w, uid)
    assert_equal(got, want, f"{kind} bias={bias} NI={NI} n={n} D={D}")
    assert np.isnan(got["auc"][0]) and np.isnan(got["recall"][0]).all()       # no positives: 0 / 0
    if n > 3 and NI <= 4099 and len(pos[3]):
        assert np.isnan(got["auc"][3])                                           # n_eval = 0


@pytest.mark.parametrize("kind", ["dot", "l2", "gmf"])
def test_one_case_per_kind_against_the_oracle(kind):
    rt = _rt()
    from oracle import metrics_oracle as mo
    NU, NI, n, D = 100, 1000, 37, 24
    U, V, b, w = tables(rt, NU, NI, D, True, seed=5)
    rng = np.random.default_rng(9)
    uid = rng.integers(0, NU, n).astype(np.int32)
    pos, excl = make_lists(rng, n, NI, 64, full_excl=False)
    pm, em = rt.SparseMask.from_lists(pos, NI), rt.SparseMask.from_lists(excl, NI)
    ww = w if kind == "gmf" else None
    got = rt.rank_metrics_matrixfree(pm, em, AT, kind, U, V, b, uid, w=ww)
    S = rt.score_all_items(kind, U, V, b, uid, w=ww)
    P, E = pm._dense(), em._dense()
    np.testing.assert_allclose(got["auc"], mo.auc(P, S, E), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got["ndcg"], mo.ndcg(P, S, E, at=AT), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got["recall"], mo.recall(P, S, E, at=AT), rtol=1e-5, atol=1e-6)


def _bias_rows(name, NI):
    j = np.arange(NI)
    if name == "ties":
        return np.full(NI, 0.25, np.float32)
    if name == "neighbours":
        return np.where(j % 2 == 0, np.float32(0.5), np.nextafter(np.float32(0.5), np.float32(1))).astype(np.float32)
    if name == "overflow":
        return (89.0 + (j % 97) * 0.25).astype(np.float32)
    if name == "underflow":
        return (-88.0 - (j % 131) * 0.25).astype(np.float32)
    raise KeyError(name)


@pytest.mark.parametrize("kind", ["dot", "gmf"])
@pytest.mark.parametrize("spot", ["ties", "neighbours", "overflow", "underflow", "scaled", "duplicates"])
def test_scores_at_the_hard_spots(spot, kind):
    """user vectors of zero make the score the bias exactly: ties, neighbouring floats, expf overflow and underflow; tables
    scaled by 1e-2 put neighbouring scores closer than 1e-6; duplicated item rows tie whole groups"""
    rt = _rt()
    NU, NI, n, D = 50, 4099, 37, 24
    rng = np.random.default_rng(11)
    U, V, b, w = tables(rt, NU, NI, D, True, seed=3, scale=0.3e-2 if spot == "scaled" else 0.3)
    if spot in ("ties", "neighbours", "overflow", "underflow"):
        U.write(np.zeros((NU, D), np.float32))
        b.write(_bias_rows(spot, NI).reshape(NI, 1))
    elif spot == "scaled":
        b = None
    else:
        Vh = V.read(); bh = b.read()
        V.write(Vh[np.arange(NI) % 50]); b.write(bh[np.arange(NI) % 50])
    uid = rng.integers(0, NU, n).astype(np.int32)
    pos, excl = make_lists(rng, n, NI, 150)
    got, want = both(rt, pos, excl, NI, kind, U, V, b, w, uid)
    assert_equal(got, want, f"{spot} {kind}")


def _budget_for(rt, n, NI, D, kind, max_pos, max_excl, batches):
    """a scratch budget under which the call takes at least `batches` batches"""
    lo = 1
    full, _ = rt.rank_metrics_matrixfree_scratch(n, NI, D, kind, max_pos, max_excl)
    hi = full
    while lo < hi:                                               # the largest budget that still needs that many batches
        mid = (lo + hi + 1) // 2
        _, per = rt.rank_metrics_matrixfree_scratch(n, NI, D, kind, max_pos, max_excl, mid)
        if -(-n // per) >= batches: lo = mid
        else: hi = mid - 1
    return lo


@pytest.mark.parametrize("kind", ["dot", "l2"])
def test_batches_equal_one_batch(kind):
    rt = _rt()
    NU, NI, n, D = 200, 4099, 130, 24
    U, V, b, w = tables(rt, NU, NI, D, True, seed=21)
    rng = np.random.default_rng(22)
    uid = rng.integers(0, NU, n).astype(np.int32)
    pos, excl = make_lists(rng, n, NI, 150, full_excl=False)
    mp, me = max(map(len, pos)), max(map(len, excl))
    budget = _budget_for(rt, n, NI, D, kind, mp, me, 3)
    _, per = rt.rank_metrics_matrixfree_scratch(n, NI, D, kind, mp, me, budget)
    assert -(-n // per) >= 3, per
    one, want = both(rt, pos, excl, NI, kind, U, V, b, w, uid)
    many, _ = both(rt, pos, excl, NI, kind, U, V, b, w, uid, scratch_bytes=budget)
    assert_equal(one, want, f"{kind} one batch")
    assert_equal(many, one, f"{kind} {-(-n // per)} batches")


def test_dense_route_batches_after_a_failed_csr_call():
    """L2 takes the dense route: the CSR metrics batch of rank_metrics_csr, once per batch.  Two batches of the wide tile shape
    (65 .. 129 of 130 users each), positive lists of 0 / 7 / 8 / 16 / 70 items (8, 16 and 64 buckets among the users, the call's
    chunking from the longest), right after a rank_metrics_csr call that failed on the device: equal to rank_metrics_csr over the
    same users in one call, bit for bit."""
    rt = _rt()
    NU, NI, n, D = 150, 300, 130, 8
    U, V, b, w = tables(rt, NU, NI, D, True, seed=41)
    rng = np.random.default_rng(42)
    uid = rng.integers(0, NU, n).astype(np.int32)
    lengths = (0, 7, 8, 16, 70)
    pos = [np.sort(rng.choice(NI, lengths[q % len(lengths)], replace=False)) for q in range(n)]
    excl = [np.setdiff1d(rng.choice(NI, int(rng.integers(0, 40)), replace=False), pos[q]) for q in range(n)]
    pm, em = rt.SparseMask.from_lists(pos, NI), rt.SparseMask.from_lists(excl, NI)
    mp, me = max(map(len, pos)), max(map(len, excl))
    assert mp == 70
    full, per = rt.rank_metrics_matrixfree_scratch(n, NI, D, "l2", mp, me)
    assert per == n
    lo, hi = 1, full                                             # the smallest budget that takes 65 users per batch
    while lo < hi:
        mid = (lo + hi) // 2
        if rt.rank_metrics_matrixfree_scratch(n, NI, D, "l2", mp, me, mid)[1] >= 65: hi = mid
        else: lo = mid + 1
    _, per = rt.rank_metrics_matrixfree_scratch(n, NI, D, "l2", mp, me, lo)
    assert 65 <= per <= 129, per
    want = rt.rank_metrics_csr(pm, em, AT, kind="l2", user=U, item=V, bias=b, uid=uid)
    items = pm.items.copy(); items[-1] = NI
    with pytest.raises(IndexError):
        rt.rank_metrics_csr(rt.SparseMask(pm.ptr, items, NI), em, AT, kind="l2", user=U, item=V, bias=b, uid=uid)
    got = rt.rank_metrics_matrixfree(pm, em, AT, "l2", U, V, b, uid, scratch_bytes=lo)
    assert_equal(got, want, f"l2, {per} users per batch")


def test_repeated_call_and_recovery_after_an_index_error():
    rt = _rt()
    NU, NI, n, D = 100, 4099, 70, 64
    U, V, b, w = tables(rt, NU, NI, D, True, seed=31)
    rng = np.random.default_rng(32)
    uid = rng.integers(0, NU, n).astype(np.int32)
    pos, excl = make_lists(rng, n, NI, 64)
    first, want = both(rt, pos, excl, NI, "dot", U, V, b, w, uid)
    again, _ = both(rt, pos, excl, NI, "dot", U, V, b, w, uid)
    assert_equal(first, want); assert_equal(again, first, "repeated call")
    pm, em = rt.SparseMask.from_lists(pos, NI), rt.SparseMask.from_lists(excl, NI)
    bad_uid = uid.copy(); bad_uid[5] = NU
    with pytest.raises(IndexError):
        rt.rank_metrics_matrixfree(pm, em, AT, "dot", U, V, b, bad_uid)
    items = pm.items.copy(); items[-1] = NI
    with pytest.raises(IndexError):
        rt.rank_metrics_matrixfree(rt.SparseMask(pm.ptr, items, NI), em, AT, "dot", U, V, b, uid)
    for kind in ("dot", "l2"):
        got, want = both(rt, pos, excl, NI, kind, U, V, b, w, uid)
        assert_equal(got, want, f"after the errors, {kind}")


@pytest.mark.parametrize("name", ["bpr", "bpr_nobias", "gmf", "ucml"])
def test_recommender_evaluate_without_the_score_matrix(name):
    from openrec_amd.tf2.data import Dataset
    from openrec_amd.tf2.recommenders import BPR, GMF, UCML
    rng = np.random.default_rng(41)
    NU, NI, D = 300, 2500, 32

    def raw(n):
        a = np.zeros(n, dtype=[("user_id", np.int32), ("item_id", np.int32)])
        a["user_id"] = rng.integers(0, NU, n); a["item_id"] = rng.integers(0, NI, n)
        return a
    train, val = Dataset(raw(6000), NU, NI, seed=1), Dataset(raw(900), NU, NI, seed=1)
    m = {"bpr": lambda: BPR(D, D, NU, NI), "bpr_nobias": lambda: BPR(D, D, NU, NI, use_item_bias=False),
         "gmf": lambda: GMF(D, D, NU, NI), "ucml": lambda: UCML(D, D, NU, NI)}[name]()
    seen = 0
    for batch in val.evaluation(batch_size=100, excl_datasets=[train]):
        want = m.evaluate(**batch, at=[50, 100])
        got = m.evaluate(**batch, at=[50, 100], score_matrix=False)
        assert_equal(got, want, name)
        if seen == 0:                                            # dense masks take the same route
            dense = m.evaluate(batch["user_id"], np.asarray(batch["pos_mask"]), np.asarray(batch["excl_mask"]), at=[50, 100],
                               score_matrix=False)
            assert_equal(dense, want, name + " dense masks")
        seen += len(batch["user_id"])
    assert seen > 0
