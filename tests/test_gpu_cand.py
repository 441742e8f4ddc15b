"""Scores and ranking metrics of candidate lists (orx_score_candidates, orx_rank_metrics_candidates, Recommender.score,
Recommender.evaluate(cand_mask=...)).

Scores must EQUAL `rt.score_all_items(...)[q, items]` bit for bit.  Metrics must EQUAL, bit for bit and NaN-aware,
`rt.rank_metrics_csr(pos, complement(cand))` on the same tables (the models: `m.evaluate` on the default dense-mask batches; see
the note there on the dense-mask kernel's unordered NDCG sum): both count the same integers from bit-identical scores and add
them up in the same fixed order, so no tolerance applies.  One case per kind is also held to oracle/metrics_oracle.py on
dense masks with `rt.score_all_items` scores at the tolerances of tests/test_metrics.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

AT = [1, 10, 100]
POS_COUNTS = (0, 1, 7, 8, 16, 64, 150)      # cross every STEPS form (7 / 15 / 63 thresholds) and span several chunks
LIST_LENGTHS = (0, 1, 15, 16, 17, 100)       # around the scorer's tile of 16 entries


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


def assert_equal(got, want, what=""):
    for key in ("auc", "ndcg", "recall"):
        g, x = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == x.shape, (what, key)
        if not np.array_equal(g, x, equal_nan=True):
            bad = np.nonzero(~((g == x) | (np.isnan(g) & np.isnan(x))).reshape(g.shape[0], -1).all(axis=1))[0]
            raise AssertionError(f"{what}: {key} differs for users {bad[:8]}: got {g[bad[0]]}, want {x[bad[0]]}")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ scores ---
def score_lists(rng, n, NI):
    """per-user lists in the GIVEN order: every length of LIST_LENGTHS that fits, one user with all NI items, one unordered
    list with repeats, one list that contains item NI - 1"""
    lists = []
    for q in range(n):
        L = min(NI, LIST_LENGTHS[(q + 1) % len(LIST_LENGTHS)])
        lists.append(rng.choice(NI, L, replace=False))
    lists[n // 2] = np.arange(NI)                                       # all items
    if n > 2:
        r = rng.integers(0, NI, 40)
        lists[1] = np.concatenate([r, r[:9], [NI - 1, 0, NI - 1]])      # unordered, repeats
        lists[2] = np.array([NI - 1])
    return lists


SCORE_CASES = [  # kind, bias, NI, n, D
    ("dot", True, 33, 1, 24), ("dot", False, 1000, 37, 18), ("dot", True, 4099, 130, 64), ("dot", False, 4099, 37, 128),
    ("dot", True, 1000, 130, 130),
    ("gmf", True, 4099, 37, 64), ("gmf", False, 1000, 130, 128), ("gmf", True, 33, 37, 18), ("gmf", False, 4099, 1, 24),
    ("gmf", True, 1000, 37, 130),
    ("l2", True, 4099, 130, 24), ("l2", False, 1000, 37, 64), ("l2", True, 33, 1, 18), ("l2", False, 4099, 37, 128),
    ("l2", True, 1000, 130, 130),
]


@pytest.mark.parametrize("kind,bias,NI,n,D", SCORE_CASES)
def test_scores_equal_the_scorer(kind, bias, NI, n, D):
    rt = _rt()
    NU = 300
    U, V, b, w = tables(rt, NU, NI, D, bias, seed=NI + D)
    rng = np.random.default_rng(NI + n + D)
    uid = rng.integers(0, NU, n).astype(np.int32)
    ww = w if kind == "gmf" else None
    lists = score_lists(rng, n, NI)
    cand = rt.CandidateLists.from_lists(lists, NI)
    S = rt.score_all_items(kind, U, V, b, uid, w=ww)
    want = np.concatenate([S[q, np.asarray(l, np.int64)] for q, l in enumerate(lists)]).astype(np.float32)
    got = rt.score_candidates(kind, U, V, b, uid, cand, w=ww)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(bits(got), bits(want)), np.nonzero(bits(got) != bits(want))[0][:8]
    again = rt.score_candidates(kind, U, V, b, uid, lists, w=ww)        # plain lists, and a repeated call
    assert np.array_equal(bits(again), bits(want))
    sm = rt.SparseMask.from_lists(lists, NI)                              # the sorted, distinct form
    got_sm = rt.score_candidates(kind, U, V, b, uid, sm, w=ww)
    want_sm = np.concatenate([S[q, sm.row(q)] for q in range(n)]).astype(np.float32)
    assert np.array_equal(bits(got_sm), bits(want_sm))


@pytest.mark.parametrize("kind", ["dot", "l2"])
def test_scores_left_on_the_device(kind):
    torch = pytest.importorskip("torch")
    rt = _rt()
    NU, NI, n, D = 100, 1000, 37, 64
    U, V, b, w = tables(rt, NU, NI, D, True, seed=2)
    rng = np.random.default_rng(6)
    uid = rng.integers(0, NU, n).astype(np.int32)
    lists = score_lists(rng, n, NI)
    want = rt.score_candidates(kind, U, V, b, uid, lists)
    got = rt.score_candidates(kind, U, V, b, uid, lists, device=True)
    assert isinstance(got, torch.Tensor) and got.is_cuda
    U.ctx.synchronize()
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))


def test_all_lists_empty():
    rt = _rt()
    U, V, b, w = tables(rt, 10, 33, 24, True, seed=1)
    uid = np.arange(3, dtype=np.int32)
    assert rt.score_candidates("dot", U, V, b, uid, [[], [], []]).shape == (0,)


# ----------------------------------------------------------------------------------------------------------- metrics ---
def metric_lists(rng, n, NI, max_pos):
    """positives / candidates per user: every count of POS_COUNTS that fits; candidates = the positives plus negatives of
    every length of LIST_LENGTHS.  Among them: a user with no positives, a candidate list that contains item NI - 1, a
    positive outside cand, candidates that are all positives (n_eval = 0), an empty cand, cand = every item."""
    counts = [c for c in POS_COUNTS if c <= max_pos and c <= NI // 2]
    pos, cand = [], []
    for q in range(n):
        c = counts[(q + 1) % len(counts)]
        p = rng.choice(NI, c, replace=False)
        neg = rng.choice(NI, min(NI, LIST_LENGTHS[(q + 2) % len(LIST_LENGTHS)] + 3 * (q % 4)), replace=False)
        pos.append(np.unique(p)); cand.append(np.union1d(p, neg))
    if n == 1:
        return pos, cand
    pos[0] = np.zeros(0, np.int64)                                       # no positives: NaN
    cand[1] = np.union1d(cand[1], [NI - 1])
    pos[2] = np.union1d(pos[2], [3, 5])[:max(2, max_pos)]; cand[2] = np.setdiff1d(np.union1d(cand[2], [4]), [3])   # 3: a positive outside cand
    if n > 5:
        cand[3] = pos[3].copy()                                          # n_eval = 0
        cand[4] = np.zeros(0, np.int64)                                  # empty cand (its positives are all outside)
        cand[5] = np.arange(NI)                                          # every item
    return pos, cand


def complement(rt, cand, NI):
    return rt.SparseMask.from_lists([np.setdiff1d(np.arange(NI), c) for c in cand], NI)


def both(rt, pos, cand, NI, kind, U, V, b, w, uid, **kw):
    pm, cm = rt.SparseMask.from_lists(pos, NI), rt.SparseMask.from_lists(cand, NI)
    ww = w if kind == "gmf" else None
    want = rt.rank_metrics_csr(pm, complement(rt, cand, NI), AT, kind=kind, user=U, item=V, bias=b, w=ww, uid=uid)
    got = rt.rank_metrics_candidates(pm, cm, AT, kind, U, V, b, uid, w=ww, **kw)
    return got, want


METRIC_CASES = [  # kind, bias, NI, n, D, longest positive list
    ("dot", True, 33, 1, 24, 7), ("dot", False, 1000, 37, 18, 16), ("dot", True, 4099, 130, 64, 150),
    ("dot", False, 4099, 37, 128, 8), ("dot", True, 1000, 130, 130, 64),
    ("gmf", True, 4099, 37, 64, 150), ("gmf", False, 1000, 130, 128, 64), ("gmf", True, 33, 37, 18, 7),
    ("gmf", False, 4099, 130, 24, 16),
    ("l2", True, 4099, 130, 24, 150), ("l2", False, 1000, 37, 64, 16), ("l2", True, 33, 1, 18, 7), ("l2", True, 1000, 37, 130, 64),
]


@pytest.mark.parametrize("kind,bias,NI,n,D,max_pos", METRIC_CASES)
def test_metrics_equal_the_complement_exclusions(kind, bias, NI, n, D, max_pos):
    rt = _rt()
    NU = 300
    U, V, b, w = tables(rt, NU, NI, D, bias, seed=NI + D)
    rng = np.random.default_rng(NI + n)
    uid = rng.integers(0, NU, n).astype(np.int32)
    pos, cand = metric_lists(rng, n, NI, max_pos)
    got, want = both(rt, pos, cand, NI, kind, U, V, b, w, uid)
    assert_equal(got, want, f"{kind} bias={bias} NI={NI} n={n} D={D}")
    if n > 5:
        assert np.isnan(got["auc"][0]) and np.isnan(got["recall"][0]).all()   # no positives: 0 / 0
        if len(pos[3]):
            assert np.isnan(got["auc"][3])                                       # n_eval = 0
        assert np.isnan(got["auc"][4])                                           # empty cand
    again, _ = both(rt, pos, cand, NI, kind, U, V, b, w, uid)
    assert_equal(again, got, "repeated call")


@pytest.mark.parametrize("kind", ["dot", "l2", "gmf"])
def test_one_case_per_kind_against_the_oracle(kind):
    rt = _rt()
    from oracle import metrics_oracle as mo
    NU, NI, n, D = 100, 1000, 37, 24
    U, V, b, w = tables(rt, NU, NI, D, True, seed=5)
    rng = np.random.default_rng(9)
    uid = rng.integers(0, NU, n).astype(np.int32)
    pos, cand = metric_lists(rng, n, NI, 64)
    pm, cm = rt.SparseMask.from_lists(pos, NI), rt.SparseMask.from_lists(cand, NI)
    ww = w if kind == "gmf" else None
    got = rt.rank_metrics_candidates(pm, cm, AT, kind, U, V, b, uid, w=ww)
    S = rt.score_all_items(kind, U, V, b, uid, w=ww)
    P, E = pm._dense(), ~cm._dense()
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
def test_metrics_at_the_hard_spots(spot, kind):
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
    pos, cand = metric_lists(rng, n, NI, 150)
    for q in range(6, n, 3):                                             # longer lists too: more ties per threshold
        cand[q] = np.union1d(cand[q], rng.choice(NI, 700, replace=False))
    got, want = both(rt, pos, cand, NI, kind, U, V, b, w, uid)
    assert_equal(got, want, f"{spot} {kind}")


def test_a_candidate_list_longer_than_one_lds_piece():
    rt = _rt()
    NU, NI, n, D = 50, 4099, 7, 24
    U, V, b, w = tables(rt, NU, NI, D, True, seed=13)
    rng = np.random.default_rng(14)
    uid = rng.integers(0, NU, n).astype(np.int32)
    pos = [np.unique(rng.choice(NI, c, replace=False)) for c in (150, 64, 7, 150, 1, 16, 70)]
    cand = [np.union1d(p[: len(p) // 2 + 1], rng.choice(NI, L, replace=False)) for p, L in zip(pos, (4000, 2047, 2048, 2049, 3000, 100, 4099))]
    got, want = both(rt, pos, cand, NI, "dot", U, V, b, w, uid)
    assert_equal(got, want, "long lists")


@pytest.mark.parametrize("kind,n", [("dot", 130), ("l2", 200)])
def test_batches_equal_one_batch(kind, n):
    rt = _rt()
    NU, NI, D = 200, 4099, 24
    U, V, b, w = tables(rt, NU, NI, D, True, seed=21)
    rng = np.random.default_rng(22)
    uid = rng.integers(0, NU, n).astype(np.int32)
    pos, cand = metric_lists(rng, n, NI, 150)
    entries = sum(map(len, pos)) + sum(map(len, cand))
    # a batch holds its list entries and their scores (8 bytes each) and on the dense route a score row per user, so under
    # these budgets a batch has less than a quarter of the entries (dot) or at most 70 of the 200 users (l2): 3 batches at least
    budget = 8 * entries // 4 if kind == "dot" else 70 * NI * 4
    one, want = both(rt, pos, cand, NI, kind, U, V, b, w, uid)
    many, _ = both(rt, pos, cand, NI, kind, U, V, b, w, uid, scratch_bytes=budget)
    assert_equal(one, want, f"{kind} one batch")
    assert_equal(many, one, f"{kind} several batches")


def test_index_errors_and_recovery():
    rt = _rt()
    NU, NI, n, D = 100, 4099, 37, 64
    U, V, b, w = tables(rt, NU, NI, D, True, seed=31)
    rng = np.random.default_rng(32)
    uid = rng.integers(0, NU, n).astype(np.int32)
    pos, cand = metric_lists(rng, n, NI, 64)
    pm, cm = rt.SparseMask.from_lists(pos, NI), rt.SparseMask.from_lists(cand, NI)
    bad_uid = uid.copy(); bad_uid[5] = NU
    items = cm.items.copy(); items[-1] = NI
    bad_cm = rt.SparseMask(cm.ptr, items, NI)
    with pytest.raises(IndexError):
        rt.rank_metrics_candidates(pm, cm, AT, "dot", U, V, b, bad_uid)
    with pytest.raises(IndexError):
        rt.rank_metrics_candidates(pm, bad_cm, AT, "dot", U, V, b, uid)
    with pytest.raises(IndexError):
        rt.score_candidates("dot", U, V, b, bad_uid, cm)
    with pytest.raises(IndexError):
        rt.score_candidates("dot", U, V, b, uid, bad_cm)
    with pytest.raises(ValueError):                                      # an unsorted row names its user and list
        rt.rank_metrics_candidates(pm, rt.CandidateLists.from_lists([c[::-1] for c in cand], NI), AT, "dot", U, V, b, uid)
    for kind in ("dot", "l2"):
        got, want = both(rt, pos, cand, NI, kind, U, V, b, w, uid)
        assert_equal(got, want, f"after the errors, {kind}")
        S = rt.score_all_items(kind, U, V, b, uid)
        flat = rt.score_candidates(kind, U, V, b, uid, cm)
        assert np.array_equal(bits(flat), bits(np.concatenate([S[q, cm.row(q)] for q in range(n)])))


# ------------------------------------------------------------------------------------------------------------ models ---
@pytest.mark.parametrize("name", ["bpr", "bpr_nobias", "gmf", "ucml"])
def test_recommender_evaluate_and_score_on_candidates(name):
    from openrec_amd.tf2.data import Dataset
    from openrec_amd.tf2.recommenders import BPR, GMF, UCML
    rng = np.random.default_rng(41)
    NU, NI, D = 300, 2500, 32

    def raw(n):
        a = np.zeros(n, dtype=[("user_id", np.int32), ("item_id", np.int32)])
        a["user_id"] = rng.integers(0, NU, n); a["item_id"] = rng.integers(0, NI, n)
        return a
    np.random.seed(5)
    train = Dataset(raw(6000), NU, NI, seed=1)
    val = Dataset(raw(900), NU, NI, num_negatives=20, seed=1)
    m = {"bpr": lambda: BPR(D, D, NU, NI), "bpr_nobias": lambda: BPR(D, D, NU, NI, use_item_bias=False),
         "gmf": lambda: GMF(D, D, NU, NI), "ucml": lambda: UCML(D, D, NU, NI)}[name]()
    seen = 0
    from openrec_amd import runtime as rt
    for dense, batch in zip(val.evaluation(100, [train]), val.evaluation(100, [train], candidates=True)):
        got = m.evaluate(**batch, at=[5, 10])
        # the default batch with its exclusion mask handed over as item lists: the fixed-order sums, equal bit for bit
        want = m.evaluate(dense["user_id"], dense["pos_mask"], rt.SparseMask.from_dense(dense["excl_mask"]), at=[5, 10])
        assert_equal(got, want, name)
        # the default batch as it comes (a dense exclusion mask takes rank_metrics_kernel): AUC and Recall are one division of
        # exact integer counts and must be equal bit for bit.  That kernel adds a user's NDCG terms with float atomics in no
        # fixed order (the order its positives were compacted in), so NDCG is held to the error of
        # re-ordering a float sum of m = n_pos terms in (0, 1], twice (m - 1) u S / (1 - (m - 1) u) with u = 2^-24 -- measured:
        # users 70 and 77 of the first bpr batch, 1.4463947 against 1.4463946, one ulp
        asis = m.evaluate(**dense, at=[5, 10])
        assert_equal({k: got[k] for k in ("auc", "recall")} | {"ndcg": asis["ndcg"]}, asis, name + " dense mask")
        g = np.maximum(np.diff(batch["pos_mask"].ptr) - 1, 0)[:, None] * 2.0 ** -24
        bound = 2 * g / (1 - g) * np.maximum(got["ndcg"], asis["ndcg"]).astype(np.float64)
        err = np.abs(got["ndcg"].astype(np.float64) - asis["ndcg"].astype(np.float64))
        assert (err <= bound).all(), (name, np.nonzero(err > bound), err.max())
        if seen == 0:
            with pytest.raises(ValueError):
                m.evaluate(batch["user_id"], batch["pos_mask"], excl_mask=dense["excl_mask"], cand_mask=batch["cand_mask"])
            cm = batch["cand_mask"]
            lists = [cm.row(q)[::-1] for q in range(cm.shape[0])]        # a re-ranker's order is not ascending
            scores = m.score(batch["user_id"], lists)
            S = np.asarray(m.inference(batch["user_id"]))
            assert len(scores) == len(lists)
            for q, (l, s) in enumerate(zip(lists, scores)):
                assert np.array_equal(bits(s), bits(S[q, l])), (name, q)
        seen += len(batch["user_id"])
    assert seen > 0
