"""CPU: the NumPy reference of the full softmax with label sets (tests/labelsets_ref.py) checked against itself -- gradients
against central differences, sets of one against tests/fullsoftmax_ref.py, float32 inside the row bound --, the autoencoder data
helpers, and the runtime's refusals of the `labels=` arguments (tests/runtime_standin.py: no library, no device)."""
import numpy as np
import pytest

import fullsoftmax_cases as fc
import fullsoftmax_ref as fr
import labelsets_cases as lc
import labelsets_ref as lr
import runtime_standin as rs
import seqrec_ref as sr


def _f64(x):
    return None if x is None else np.asarray(x).astype(np.float64)


def _small(bias=True, seed=5):
    case = dict(opt="sgd", bias=bias, B=9, D=5, NU=7, NI=11, chunk_items=0, chunk_samples=0, seed=seed, name="fd")
    _, V, b, _, _ = fc.make(case)
    rng = np.random.default_rng(seed)
    Q = rng.uniform(-1, 1, (case["B"], case["D"]))
    lptr, litems, lw = lc.make_sets(case, weights=True, lens=[0, 1, 2, 3, 4, 5, 6, 2, 1])
    w = rng.uniform(0.5, 1.5, case["B"])
    off = rng.normal(0, 1, case["NI"])
    return Q, _f64(V), _f64(b), lptr, litems, _f64(lw), w, off


@pytest.mark.parametrize("bias", [True, False])
def test_the_float64_gradients_are_the_central_differences_of_the_loss(bias):
    Q, V, b, lptr, litems, lw, w, off = _small(bias)
    scale, l2 = 1.5, 0.03

    def J(Q, V, b):
        loss, l2_loss = lr.forward_q(Q, V, b, lptr, litems, lw, w, off, scale)
        return loss + l2 * l2_loss

    g = lr.grads_q(Q, V, b, lptr, litems, lw, w, off, scale, l2)
    h = 1e-6
    for name, X, G in (("gu", Q, g["gu"]), ("GV", V, g["GV"])) + ((("Gb", b, g["Gb"][:, None]),) if bias else ()):
        num = np.zeros_like(X)
        for idx in np.ndindex(*X.shape):
            keep = X[idx]
            X[idx] = keep + h; up = J(Q, V, b)
            X[idx] = keep - h; dn = J(Q, V, b)
            X[idx] = keep
            num[idx] = (up - dn) / (2 * h)
        err = np.abs(num - G).max()
        print(f"{name}: max |central difference - gradient| {err:.3g}")
        assert err <= 1e-8, name


def test_the_empty_set_keeps_its_l2_part_alone():
    Q, V, b, lptr, litems, lw, w, off = _small()
    g = lr.grads_q(Q, V, b, lptr, litems, lw, w, off, 1.0, 0.1)
    assert lptr[1] == lptr[0]
    assert np.array_equal(g["gu"][0], 0.1 * Q[0]) and lr.row_losses_q(Q, V, b, lptr, litems, lw, off)[0] == 0.0


@pytest.mark.parametrize("si", range(len(fc.SHAPES)))
def test_sets_of_one_with_unit_weights_are_the_single_label_reference(si):
    case = fc.shape_case(si, bias=si % 2 == 0)
    U, V, b, uid, pid = fc.make(case)
    Q, V, b = _f64(U)[uid], _f64(V), _f64(b)
    B = case["B"]
    rng = np.random.default_rng(si)
    w, off = rng.uniform(0, 2, B), rng.normal(0, 1, case["NI"])
    lptr = np.arange(B + 1, dtype=np.int32)
    a = lr.forward_q(Q, V, b, lptr, pid, None, w, off, 2.0)
    c = fr.forward_q(Q, V, b, pid, w, off, 2.0)
    assert np.allclose(a, c, rtol=1e-12, atol=0)
    ga = lr.grads_q(Q, V, b, lptr, pid, None, w, off, 2.0, 0.01)
    gc = fr.grads_q(Q, V, b, pid, w, off, 2.0, 0.01)
    for k in ("gu", "GV", "Gb"):
        assert np.abs(ga[k] - gc[k]).max() <= 1e-13 * max(np.abs(gc[k]).max(), 1.0), k
    # the bound of a set of one is the single-label bound plus the (1 + 2) u (|lse| + |s|) of the set's own sum
    off32 = off.astype(np.float32)
    s = fr.scores(Q, V, b, _f64(off32), 2.0)
    extra = 3 * lr.U32 * (np.abs(fr._lse(s)) + np.abs(s[np.arange(B), pid]))
    assert np.allclose(lr.row_bound_q(U[uid], V, b, lptr, pid, None, off32, 2.0), fr.row_bound_q(U[uid], V, b, pid, off32, 2.0) + extra, rtol=1e-12, atol=0)


@pytest.mark.parametrize("si", range(len(fc.SHAPES)))
def test_the_float32_reference_is_inside_the_row_bound(si):
    worst = 0.0
    for bias, weights, offset in ((True, True, True), (False, False, False)):
        case = lc.shape_case(si, bias=bias, seed=600 + si)
        H, V, b, ptr, items = lc.make_seq(case)
        lptr, litems, lw = lc.make_sets(case, weights)
        off = np.random.default_rng(si).normal(0, 1, case["NI"]).astype(np.float32) if offset else None
        for scale in (1.0, 4.0):
            got = lr.seq_row_losses(H, V, b, ptr, items, lptr, litems, "mean", lw, off, np.float32(scale)).astype(np.float64)
            # (the float32 pool rounds the query: the bound is taken on the float32 query, and the exact loss on it too)
            Q32, _ = sr.pool_rows(H, ptr, items, "mean")
            want = lr.row_losses_q(_f64(Q32), _f64(V), _f64(b), lptr, litems, _f64(lw), _f64(off), scale)
            bound = lr.row_bound_q(Q32, V, b, lptr, litems, lw, off, scale)
            live = bound > 0
            assert (np.abs(got - want)[~live] == 0).all()
            if live.any():
                worst = max(worst, float((np.abs(got - want)[live] / bound[live]).max()))
    print(f"shape {si}: worst float32 row at {worst:.3g} x bound")
    assert worst <= 1.0


# ---- the data helpers --------------------------------------------------------------------------------------------------------------
def _raw(seed=0, users=40, items=60):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 12, users)
    lens[3] = 1
    u = np.repeat(np.arange(users), lens)
    it = np.concatenate([rng.permutation(items)[:n] for n in lens]).astype(np.int64)
    perm = rng.permutation(len(u))
    return dict(user_id=u[perm], item_id=it[perm]), lens


def test_autoencoder_batches_drop_entries_keep_one_and_label_the_full_list():
    from openrec_amd.tf2.data import autoencoder_batches
    raw, lens = _raw()
    full = {u: [int(i) for uu, i in zip(raw["user_id"], raw["item_id"]) if uu == u] for u in range(40)}
    gen = autoencoder_batches(raw, 40, 64, seed=3, dropout=0.9)
    dropped_some = False
    for _ in range(5):
        bt = next(gen)
        assert bt["in_items"].dtype == np.int32 and bt["in_items"].shape == bt["label_items"].shape
        for k in range(64):
            u = int(bt["user_id"][k])
            lab = bt["label_items"][k, :bt["label_len"][k]].tolist()
            kept = bt["in_items"][k, :bt["in_len"][k]].tolist()
            assert lab == full[u] and len(lab) >= 1                         # the labels are the full list, in record order
            assert 1 <= len(kept) <= len(lab)                               # at least one entry survives
            it = iter(lab)
            assert all(x in it for x in kept)                               # a subsequence of the list
            dropped_some |= len(kept) < len(lab)
    assert dropped_some
    a, c = autoencoder_batches(raw, 40, 16, seed=9), autoencoder_batches(raw, 40, 16, seed=9)
    for _ in range(3):
        x, y = next(a), next(c)
        assert all(np.array_equal(x[k], y[k]) for k in x)
    bt = next(autoencoder_batches(raw, 40, 32, seed=1, dropout=0.0, max_len=4))
    assert np.array_equal(bt["in_items"], bt["label_items"]) and bt["label_len"].max() <= 4 and bt["label_items"].shape[1] <= 4
    with pytest.raises(ValueError):
        next(autoencoder_batches(raw, 40, 8, seed=0, dropout=1.0))


def test_autoencoder_evaluation_gives_fold_in_histories_with_their_lists():
    from openrec_amd.tf2.data import autoencoder_evaluation
    train, _ = _raw(1)
    held, _ = _raw(2)
    batches = list(autoencoder_evaluation(train, held, 40, batch_size=16))
    users = np.concatenate([bt["user_id"] for bt in batches])
    both = sorted(set(train["user_id"].tolist()) & set(held["user_id"].tolist()))
    assert users.tolist() == both
    for bt in batches:
        for k, u in enumerate(bt["user_id"]):
            hist = bt["seq_item_id"][k, :bt["seq_len"][k]].tolist()
            assert hist == [int(i) for uu, i in zip(train["user_id"], train["item_id"]) if uu == u]
            assert bt["pos_item_id"][k, :bt["pos_len"][k]].tolist() == [int(i) for uu, i in zip(held["user_id"], held["item_id"]) if uu == u]
            assert bt["excl_item_id"][k, :bt["excl_len"][k]].tolist() == hist


# ---- the runtime's refusals --------------------------------------------------------------------------------------------------------
def _call(dev=False, **over):
    from openrec_amd import runtime as rt
    w = rs.World(rt)
    n = 4
    ptr = np.arange(0, 2 * n + 1, 2, dtype=np.int32)
    lists = dict(bags=(ptr, np.ones(2 * n, np.int32)), pid=None, labels=(ptr.copy(), np.ones(2 * n, np.int32)), label_weights=None)
    if dev:
        T = rs.FakeDeviceTensor
        lists = dict(bags=(T(n + 1), T(2 * n)), pid=None, labels=(T(n + 1), T(2 * n)), label_weights=None)
    lists.update(over)
    net = w.seqrec()
    net.step_full(w.opt, lists["bags"], lists["pid"], labels=lists["labels"], label_weights=lists["label_weights"])
    return w


def test_the_runtime_passes_label_sets_to_the_sets_call():
    for dev in (False, True):
        w = _call(dev)
        names = [c[0] for c in w.calls if c[0] != "check_index_error"]
        assert names == ["orx_seqrec_full_sets_step"]
        args = w.calls[0][1]
        assert args[9] is None and args[10] == 8 and args[13] == 4 and args[14] == 8       # lab_weight, n_lab, B, n
    w = _call(pid=np.ones(4, np.int32), labels=None)
    assert [c[0] for c in w.calls if c[0] != "check_index_error"] == ["orx_seqrec_full_step"]
    w = _call(label_weights=np.ones(8, np.float32))
    assert w.calls[0][1][9] is not None


def test_the_runtime_refuses_bad_label_arguments_before_the_library_is_called():
    T = rs.FakeDeviceTensor
    ptr = np.arange(0, 9, 2, dtype=np.int32)
    bad = [dict(pid=np.ones(4, np.int32)),                                                   # both
           dict(labels=None),                                                                # neither
           dict(pid=np.ones(4, np.int32), labels=None, label_weights=np.ones(4, np.float32)),  # weights without sets
           dict(labels=(np.arange(0, 7, 2, dtype=np.int32), np.ones(6, np.int32))),          # three sets for four bags
           dict(labels=(ptr[::-1].copy(), np.ones(8, np.int32))),                            # a decreasing host ptr
           dict(labels=(ptr, np.ones(7, np.int32))),                                         # ptr[B] != n_lab
           dict(labels=(T(5), T(8))),                                                        # on the device beside host bags
           dict(label_weights=np.ones(7, np.float32)),                                       # one weight short
           dict(label_weights=T(8, "float32")),                                              # weights on the other side
           dict(labels=ptr)]                                                                 # not a pair
    for over in bad:
        from openrec_amd import runtime as rt
        w = rs.World(rt)
        lists = dict(bags=(ptr, np.ones(8, np.int32)), pid=None, labels=(ptr.copy(), np.ones(8, np.int32)), label_weights=None)
        lists.update(over)
        with pytest.raises(ValueError):
            w.seqrec().step_full(w.opt, lists["bags"], lists["pid"], labels=lists["labels"], label_weights=lists["label_weights"])
        assert not w.calls, over
