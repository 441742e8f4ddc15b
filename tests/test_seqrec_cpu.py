"""CPU: the history-pooled sequence recommender's reference and host code.  tests/seqrec_ref.py against torch float64 autograd of
the written objective; the padded-to-ragged conversion; the ValueErrors of the runtime layer, raised without the library; the
temporal batch generators; and the headroom of seqrec_ref.pool_bound for a float32 NumPy pooling of the cases."""
import itertools

import numpy as np
import pytest

import seqrec_cases as sc
import seqrec_ref as sr

POOLS = ("mean", "sum", sc.FIXED)


def _rt():
    from openrec_amd import runtime as rt
    return rt


# ---- the reference's gradients are the objective's ---------------------------------------------------------------------------------------
def _torch_objective(kind, H, V, b, ptr, items, pid, nid, pool, w, off, l2_reg):
    import torch
    B, N = nid.shape
    own = torch.from_numpy(sr.owners(ptr))
    lens = torch.from_numpy(np.diff(ptr).astype(np.float64))
    S = torch.zeros((B, H.shape[1]), dtype=torch.float64).index_add(0, own, H[torch.from_numpy(items.astype(np.int64))])
    if pool == "mean":
        c = torch.where(lens > 0, 1.0 / torch.clamp(lens, min=1.0), torch.zeros_like(lens))
    else:
        c = torch.full_like(lens, 1.0 if pool == "sum" else 1.0 / pool[1])
    Q = c[:, None] * S
    p, n = V[torch.from_numpy(pid.astype(np.int64))], V[torch.from_numpy(nid.astype(np.int64))]
    sp = (Q * p).sum(1) + b[torch.from_numpy(pid.astype(np.int64)), 0]
    s = (Q[:, None, :] * n).sum(2) + b[torch.from_numpy(nid.astype(np.int64)), 0] + torch.from_numpy(off)
    if kind == "softmax":
        l = torch.logsumexp(torch.cat([sp[:, None], s], 1), 1) - sp
    else:
        l = -torch.nn.functional.logsigmoid(torch.clamp(sp[:, None] - s, min=-30.0)).mean(1)
    loss = (torch.from_numpy(w) * l).sum() / B
    l2 = 0.5 * ((Q * Q).sum() + (p * p).sum() + (n * n).sum())
    return loss + l2_reg * l2, loss, l2


@pytest.mark.parametrize("kind", sr.KINDS)
@pytest.mark.parametrize("pool", POOLS, ids=sc._pool_name)
def test_reference_gradients_are_autograd_of_the_written_objective(kind, pool):
    import torch
    rng = np.random.default_rng(3)
    NI, D, B, N, l2_reg = 50, 6, 40, 5, 0.3
    H, V, b = (rng.uniform(-0.5, 0.5, s) for s in ((NI, D), (NI, D), (NI, 1)))
    ptr, items = sc.make_bags(rng, B, NI)
    pid = rng.integers(0, NI, B).astype(np.int32); nid = rng.integers(0, NI, (B, N)).astype(np.int32)
    w = rng.uniform(0, 2, B); w[::5] = 0.0
    off = rng.normal(0, 1, (B, N)); off[:, 1] = -np.inf
    tH, tV, tb = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (H, V, b))
    J, loss, l2 = _torch_objective(kind, tH, tV, tb, ptr, items, pid, nid, pool, w, off, l2_reg)
    J.backward()
    got_loss, got_l2 = sr.forward(kind, H, V, b, ptr, items, pid, nid, pool, w, off)
    assert abs(got_loss - loss.item()) <= 1e-12 * abs(loss.item()) and abs(got_l2 - l2.item()) <= 1e-12 * abs(l2.item())
    g = sr.grads(kind, H, V, b, ptr, items, pid, nid, pool, w, off, l2_reg)
    ids = np.concatenate([pid, nid.reshape(-1)])
    dH = np.zeros_like(H); np.add.at(dH, items, g["gh"])
    dV = np.zeros_like(V); np.add.at(dV, ids, np.concatenate([g["gp"], g["gn"].reshape(-1, D)]))
    db = np.zeros_like(b); np.add.at(db[:, 0], ids, np.concatenate([g["gbp"], g["gbn"].reshape(-1)]))
    for name, got, want in (("H", dH, tH.grad.numpy()), ("V", dV, tV.grad.numpy()), ("b", db, tb.grad.numpy())):
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"{kind} {sc._pool_name(pool)} d{name}: rel err {err:.3g}")
        assert err <= 1e-10, name


def test_reference_step_is_the_optimizers_on_the_occurrence_rows():
    """one SGD step of the reference moves every table by -lr times the dense gradient"""
    from oracle import numpy_oracle as orc
    rng = np.random.default_rng(4)
    NI, D, B, N = 40, 5, 30, 4
    H, V, b = (rng.uniform(-0.5, 0.5, s) for s in ((NI, D), (NI, D), (NI, 1)))
    ptr, items = sc.make_bags(rng, B, NI)
    pid = rng.integers(0, NI, B).astype(np.int32); nid = rng.integers(0, NI, (B, N)).astype(np.int32)
    g = sr.grads("softmax", H, V, b, ptr, items, pid, nid, "mean", l2_reg=0.1)
    dH = np.zeros_like(H); np.add.at(dH, items, g["gh"])
    H1, V1, b1 = H.copy(), V.copy(), b.copy()
    sr.step("softmax", H1, V1, b1, ptr, items, pid, nid, orc.SGD(0.05), "mean", l2_reg=0.1)
    assert np.allclose(H1, H - 0.05 * dH, rtol=0, atol=1e-14) and not np.array_equal(V1, V) and not np.array_equal(b1, b)


class _SummingSGD:
    """SGD that sums a row's occurrences first, in list order at the table's dtype, as the sorted apply does"""

    def __init__(self, lr):
        self.lr = lr

    def apply(self, W, ids, G, key=None):
        S = np.zeros_like(W)
        np.add.at(S, ids, G.astype(W.dtype))
        rows = np.unique(ids)
        W[rows] -= W.dtype.type(self.lr) * S[rows]


@pytest.mark.parametrize("case", sc.CASES, ids=[c["name"] for c in sc.CASES])
def test_cases_leave_room_for_a_float32_implementation(case):
    """one step of seqrec_ref at float32 against float64, under the measure of tests/test_gpu_seqrec.py: within 0.6 of
    conftest.delta_check's bound (Adam: of TOL_ADAM) on every table"""
    import multineg_cases as mc
    from conftest import TOL_ADAM, rel_err
    H, V, b = sc.make_tables(case)
    bt = sc.make_batches(case)[0]
    l2_reg = 0.01 if case["seed"] % 2 else 0.0
    res = {}
    for dt in (np.float64, np.float32):
        tabs = [x.astype(dt) if x is not None else None for x in (H, V, b)]
        oo = _SummingSGD(mc.LR["sgd"]) if case["opt"] == "sgd" else mc.make_opt(case["opt"])
        w, off = (None if x is None else x.astype(dt) for x in (bt["w"], bt["off"]))
        sr.step(case["kind"], *tabs, bt["ptr"], bt["items"], bt["pid"], bt["nid"], oo, case["pool"], w=w, off=off, l2_reg=l2_reg)
        res[dt] = tabs
    for name, W0, got, want in zip(("history", "item", "bias"), (H, V, b), res[np.float32], res[np.float64]):
        if W0 is None:
            continue
        got, want = got.astype(np.float32), want.astype(np.float32)
        if case["opt"] == "adam":
            ratio = rel_err(got, want) / TOL_ADAM
        else:
            d_got, d_want = got.astype(np.float64) - W0, want.astype(np.float64) - W0
            ulp = np.spacing(np.maximum(np.maximum(np.abs(want), np.abs(W0)), np.float32(np.abs(d_want).max())))
            ratio = float((np.abs(d_got - d_want) / (1e-5 * np.abs(d_want) + 2 * ulp.astype(np.float64))).max())
        print(f"{case['name']} {name}: {ratio:.2f} of the bound")
        assert ratio <= 0.6, name


# ---- padded -> ragged ------------------------------------------------------------------------------------------------------------------------
def test_padded_to_ragged_never_reads_the_padding():
    rt = _rt()
    rng = np.random.default_rng(5)
    ptr, items = sc.make_bags(rng, 64, 100)
    lens = np.diff(ptr)
    L = int(lens.max()) + 2
    for fill in (-1, 2 ** 31 - 1, -2 ** 31):
        seq = np.full((64, L), fill, np.int64)
        for i, n in enumerate(lens):
            seq[i, :n] = items[ptr[i]:ptr[i + 1]]
        p, it = rt.bags_to_ragged(seq, lens)
        assert p.dtype == np.int32 and it.dtype == np.int32 and np.array_equal(p, ptr) and np.array_equal(it, items)
        p2, it2 = rt.bags_to_ragged(seq.astype(np.int32), lens.astype(np.int32))
        assert np.array_equal(p2, ptr) and np.array_equal(it2, items)
    p, it = rt.bags_to_ragged(np.zeros((3, 4), np.int32), np.zeros(3, np.int32))
    assert np.array_equal(p, [0, 0, 0, 0]) and it.size == 0
    for bad in (np.array([1, 5, 0]), np.array([1, -1, 0]), np.array([1, 1])):
        with pytest.raises(ValueError):
            rt.bags_to_ragged(np.zeros((3, 4), np.int32), bad)
    with pytest.raises(ValueError):
        rt.bags_to_ragged(np.zeros(4, np.int32), np.zeros(4, np.int32))


# ---- ValueErrors before the library ----------------------------------------------------------------------------------------------------------
from runtime_standin import NoDevice as _NoDevice


class _T:
    """a stand-in table: the wrappers' checks read these fields only"""

    def __init__(self, rows, dim, ctx):
        self.rows, self.dim, self.ctx, self.shape = rows, dim, ctx, (rows, dim)

    def __getattr__(self, name):
        raise AssertionError(f"the runtime reached for .{name} before it refused the call")


def test_bad_arguments_raise_value_errors_without_the_library():
    rt = _rt()
    ctx = _NoDevice()
    H, V, b = _T(50, 8, ctx), _T(50, 8, ctx), _T(50, 1, ctx)
    opt = _NoDevice()
    ptr = np.array([0, 2, 2, 5], np.int32); items = np.array([1, 2, 3, 4, 5], np.int32)
    pid = np.array([1, 2, 3], np.int32); nid = np.zeros((3, 4), np.int32)
    # the constructor
    for args, kw in (((H, H, None), {}), ((H, _T(50, 9, ctx), None), {}), ((H, _T(51, 8, ctx), None), {}),
                     ((_T(50, 257, ctx), _T(50, 257, ctx), None), {}), ((H, V, _T(50, 2, ctx)), {}), ((H, V, _T(49, 1, ctx)), {}),
                     ((H, _T(50, 8, _NoDevice()), None), {}), ((H, V, b), dict(pool="max")), ((H, V, b), dict(pool=("fixed", 0))),
                     ((H, V, b), dict(pool=("fixed", float("inf")))), ((H, V, b), dict(pool=("fixed", -2.0))), ((H, V, b), dict(pool=("mean", 3)))):
        with pytest.raises(ValueError):
            rt.SeqRec(*args, **kw)
    net = rt.SeqRec(H, V, b, pool=("fixed", 20))
    nob = rt.SeqRec(H, V, None, pool="sum")
    good = dict(bags=(ptr, items), pid=pid, nid=nid)
    bad = [dict(good, loss="hinge"),
           dict(good, nid=np.zeros(12, np.int32)), dict(good, nid=np.zeros((3, 0), np.int32)), dict(good, nid=np.zeros((3, 65), np.int32)),
           dict(good, nid=np.zeros((2, 4), np.int32)), dict(good, pid=pid[:2]),
           dict(good, bags=(np.array([1, 2, 2, 5], np.int32), items)), dict(good, bags=(np.array([0, 3, 2, 5], np.int32), items)),
           dict(good, bags=(np.array([0, 2, 2, 4], np.int32), items)), dict(good, bags=(ptr, items, items)), dict(good, bags=ptr),
           dict(good, bags=(np.zeros((3, 2), np.int32), np.array([1, 3, 0]))),
           dict(good, weights=np.ones(2, np.float32)), dict(good, neg_offset=np.zeros((3, 3), np.float32)),
           dict(good, l2_reg=-1.0), dict(good, l2_reg=float("nan")),
           dict(good, train=("user",)), dict(good, train=()), dict(good, train=("history", "proj"))]
    for kw in bad:
        with pytest.raises(ValueError):
            net.step(opt, **kw)
    with pytest.raises(ValueError):
        nob.step(opt, train=("bias",), **good)
    for kw in bad[:14]:
        with pytest.raises(ValueError):
            net.loss(**kw)
    out = _T(10, 8, ctx)
    for args, kw in (((H, (ptr, items), H), {}), ((H, (ptr, items), _T(10, 9, ctx)), {}), ((H, (ptr, items), out), dict(pool="avg")),
                     ((H, (ptr, items), out), dict(rows=(8, 3))), ((H, (ptr, items), out), dict(rows=(0, 4))), ((H, (ptr, items), out), dict(rows=(-1, 3))),
                     ((H, (np.array([0, 6], np.int32), items), out), {})):
        with pytest.raises(ValueError):
            rt.bag_pool(*args, **kw)
    with pytest.raises(ValueError):
        net.user_table((ptr, items), out=_T(4, 8, ctx))
    from openrec_amd.tf2.recommenders import vanilla_youtube_rec as vy
    assert vy.VanillaYouTubeRec.__init__.__defaults__ is not None
    for kw in (dict(dim_item_embed=0), dict(dim_item_embed=300), dict(max_seq_len=0), dict(pool="max"), dict(l2_reg_embed=-1.0)):
        with pytest.raises(ValueError):
            vy.VanillaYouTubeRec(**dict(dict(dim_item_embed=8, max_seq_len=5, total_items=20, ctx=_NoDevice()), **kw))


# ---- the temporal generators -------------------------------------------------------------------------------------------------------------------
def _raw(rng, users, items, records):
    raw = np.zeros(records, dtype=[("user_id", np.int32), ("item_id", np.int32), ("ts", np.int64)])
    raw["user_id"] = rng.integers(0, users - 3, records)           # users - 3 .. users - 1: no records at all
    raw["item_id"] = rng.integers(0, items, records)
    raw["ts"] = rng.integers(0, 50, records)                       # with ties
    raw["user_id"][raw["user_id"] == 5] = 6                        # user 5: none
    one = np.zeros(1, raw.dtype); one["user_id"], one["item_id"], one["ts"] = 5, 9, 7
    return np.concatenate([raw[:100], one, raw[100:]])             # user 5: exactly one record


@pytest.mark.parametrize("time_field", [None, "ts"])
def test_temporal_batches_follow_the_samplers_rule(time_field):
    from openrec_amd.tf2 import data
    rng = np.random.default_rng(8)
    users, L = 40, 6
    raw = _raw(rng, users, 30, 600)
    order = np.arange(len(raw)) if time_field is None else np.lexsort((np.arange(len(raw)), raw["ts"]))
    lists = {u: raw["item_id"][order][raw["user_id"][order] == u] for u in range(users)}
    a, b = data.temporal_batches(raw, users, 64, L, 11, time_field), data.temporal_batches(raw, users, 64, L, 11, time_field)
    c = data.temporal_batches(raw, users, 64, L, 12, time_field)
    seen, pos_seen = set(), set()
    for k, (x, y, z) in enumerate(itertools.islice(zip(a, b, c), 30)):
        assert all(np.array_equal(x[f], y[f]) for f in x), "the same seed gives the same batches"
        assert k > 0 or not np.array_equal(x["user_id"], z["user_id"])
        assert x["seq_item_id"].shape == (64, L) and x["seq_item_id"].dtype == np.int32 and x["seq_len"].dtype == np.int32
        for seq, n, lab, u in zip(x["seq_item_id"], x["seq_len"], x["label"], x["user_id"]):
            full = lists[int(u)]
            assert len(full) >= 2 and 1 <= n <= L and (seq[n:] == 0).all()
            # the history is the contiguous slice before some position that holds the label
            ends = [p for p in range(1, len(full)) if full[p] == lab and min(p, L) == n and np.array_equal(full[p - n:p], seq[:n])]
            assert ends, (u, seq, n, lab)
            seen.add(int(u)); pos_seen.add((int(u), ends[0]))
    warm = {u for u in range(users) if len(lists[u]) >= 2}
    assert 5 not in seen and seen == warm and len(lists[5]) == 1
    assert any(p == len(lists[u]) - 1 for u, p in pos_seen) and any(p == 1 for u, p in pos_seen)


@pytest.mark.parametrize("time_field", [None, "ts"])
def test_temporal_evaluation_takes_the_last_item_as_the_label(time_field):
    from openrec_amd.tf2 import data
    rng = np.random.default_rng(9)
    users, L = 40, 6
    raw = _raw(rng, users, 30, 600)
    order = np.arange(len(raw)) if time_field is None else np.lexsort((np.arange(len(raw)), raw["ts"]))
    lists = {u: raw["item_id"][order][raw["user_id"][order] == u] for u in range(users)}
    whole = list(data.temporal_evaluation(raw, users, L, time_field))
    assert len(whole) == 1
    parts = list(data.temporal_evaluation(raw, users, L, time_field, batch_size=7))
    for f in whole[0]:
        assert np.array_equal(whole[0][f], np.concatenate([p[f] for p in parts]))
    x = whole[0]
    assert list(x["user_id"]) == [u for u in range(users) if len(lists[u]) >= 2]
    for seq, n, lab, u in zip(x["seq_item_id"], x["seq_len"], x["label"], x["user_id"]):
        full = lists[int(u)]
        assert lab == full[-1] and n == min(len(full) - 1, L) and np.array_equal(seq[:n], full[-1 - n:-1]) and (seq[n:] == 0).all()


# ---- the bound has headroom for the reference itself --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.CASES, ids=[c["name"] for c in sc.CASES])
def test_pool_bound_holds_for_a_float32_numpy_pooling(case):
    H, _, _ = sc.make_tables(case, scale=1.0)
    bt = sc.make_batches(case)[0]
    got, _ = sr.pool_rows(H, bt["ptr"], bt["items"], case["pool"])
    assert got.dtype == np.float32
    want, c = sr.pool_rows(H.astype(np.float64), bt["ptr"], bt["items"], case["pool"])
    bound = sr.pool_bound(H, bt["ptr"], bt["items"], c)
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"{case['name']}: worst |err| / bound {ratio:.3g}")
    assert (err <= bound).all()
    empty = np.diff(bt["ptr"]) == 0
    assert not got[empty].any() and not np.signbit(got[empty]).any()
