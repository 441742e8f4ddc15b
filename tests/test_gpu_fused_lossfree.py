"""GPU: the fused pairwise step called WITHOUT loss buffers (fused_kernel LOSS = false, no loss sums behind the last step).

The loss-free kernel is the same source with the loss sums compiled out; every update's arithmetic is left alone.  So the tables are
compared BIT FOR BIT wherever two runs of ONE kernel would agree bit for bit: on every row with at most two references in a step.
A row referenced >= 3 times sums its gradients in an order no run fixes -- by fp32 atomics, or from staging slots whose ranks an
atomic counter of the plan hands out (measured: the call with the loss and the call without differed in 12 elements of one item
row, by one ulp; two runs of the call with the loss differ alike).  Where such rows occur both runs are held to the oracle instead,
by the bound the suite has for this step: TOL on the tables and conftest.delta_check on the updates.  The cases come in two forms:
  drawn    the ids as drawn, ORX_PLAN_MIN_LATE=1 (every range with a third reference stages: the STAGED kernels)
  thinned  no row has more than two references in a step (the kernels without the staging bookkeeping)
The role-coverage shape (tables of 20000 rows, B = 2048, K = 3, D = 64) shows unique rows, paired rows, twice-referenced rows whose
pair was refused, rows with >= 3 references (drawn form) and urgent references across steps; each is asserted from the ids and the
plan's counters (Context.stat), as is "the in-launch apply stayed on" (fewer than B / 5 duplicated rows left per step)."""
import os

import numpy as np
import pytest

from conftest import TOL, delta_check

pytestmark = pytest.mark.gpu

LR = 0.05


def _rt():
    from openrec_amd import runtime as rt
    return rt


class env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# every knob that changes the path of the step, pinned (None: unset) unless a case sets it
CLEAN = dict(ORX_PAIR_ALWAYS=1, ORX_NO_PAIR=None, ORX_PLAN_WAIT=None, ORX_PLAN_MIN_LATE=None,
             ORX_FORCE_FALLBACK=None, ORX_PLAN_V1=None)


def _env(**kw):
    return env(**{**CLEAN, **kw})


def _thin(ids, rows, rng):
    """at most two references per row in `ids` (1-D): every later reference moves to a row nothing references yet"""
    ids = ids.copy()
    order = np.argsort(ids, kind="stable")
    s = ids[order]
    rank = np.arange(s.size) - np.searchsorted(s, s, side="left")
    extra = order[rank >= 2]
    free = np.setdiff1d(np.arange(rows, dtype=np.int64), ids)
    assert free.size >= extra.size
    ids[extra] = rng.permutation(free)[:extra.size]
    return ids


def _case(seed, NU, NI, B, D, K, thin=False):
    rng = np.random.default_rng(seed)
    U = rng.uniform(-.05, .05, (NU, D)).astype(np.float32)
    V = rng.uniform(-.05, .05, (NI, D)).astype(np.float32)
    b = rng.uniform(-.05, .05, (NI, 1)).astype(np.float32)
    uid = rng.integers(0, NU, (K, B)).astype(np.int32)
    pid = rng.integers(0, NI, (K, B)).astype(np.int32)
    nid = rng.integers(0, NI, (K, B)).astype(np.int32)
    if thin:
        for k in range(K):
            uid[k] = _thin(uid[k], NU, rng)
            it = _thin(np.concatenate([pid[k], nid[k]]), NI, rng)
            pid[k], nid[k] = it[:B], it[B:]
    return U, V, b, uid, pid, nid


def _roles(uid, pid, nid, NU, NI):
    """per call: rows referenced once / exactly twice / >= 3 times in a step (summed over steps), and the references of a step to a
    row that the step before it referenced more than once (urgent)"""
    out = dict(unique=0, twice=0, many=0, urgent=0, dup_max=0)
    prev = None
    for k in range(uid.shape[0]):
        cu = np.bincount(uid[k], minlength=NU)
        ci = np.bincount(np.concatenate([pid[k], nid[k]]), minlength=NI)
        for c in (cu, ci):
            out["unique"] += int((c == 1).sum()); out["twice"] += int((c == 2).sum()); out["many"] += int((c >= 3).sum())
        out["dup_max"] = max(out["dup_max"], int((cu >= 2).sum() + (ci >= 2).sum()))
        if prev is not None:
            out["urgent"] += int((prev[0][uid[k]] >= 2).sum() + (prev[1][pid[k]] >= 2).sum() + (prev[1][nid[k]] >= 2).sum())
        prev = (cu, ci)
    return out


def _opt(rt, ctx, kind):
    return rt.Optimizer.sgd(LR, ctx=ctx) if kind == "sgd" else rt.Optimizer.adagrad(LR, 0.1, 1e-7, ctx=ctx)


def _run(model, U, V, b, uid, pid, nid, want_loss, censor=False, bias=True, opt="sgd", weights=None, raises=None):
    """one K-step call from fresh tables in a context of its own (the first call of a context reads its plan's counters back)"""
    rt = _rt()
    ctx = rt.Context(0)
    tU, tV = rt.Table(*U.shape, ctx).write(U), rt.Table(*V.shape, ctx).write(V)
    tb = rt.Table(*b.shape, ctx).write(b) if bias else None
    K, B = uid.shape
    kw = dict(K=K, B=B, margin=0.5, censor=censor, want_loss=want_loss)
    if weights is not None:
        kw.update(weights=weights.reshape(-1), l2_reg=0.5)
    call = lambda: rt.pairwise_step(model, _opt(rt, ctx, opt), tU, tV, tb, uid.reshape(-1), pid.reshape(-1), nid.reshape(-1), **kw)
    if raises is not None:
        with pytest.raises(raises):
            call()
        res = None
    else:
        res = call()
    assert (res is None) == (not want_loss or raises is not None)
    return dict(U=tU.read(), V=tV.read(), b=tb.read() if bias else None, loss=res, pairs=ctx.stat("pairs"), max_dup=ctx.stat("max_dup"))


def _same_tables(x, y, what):
    for k in ("U", "V", "b"):
        if x[k] is not None:
            assert np.array_equal(x[k], y[k]), "%s: %s differs in %d elements, max %.3g" % (
                what, k, int((x[k] != y[k]).sum()), float(np.abs(x[k].astype(np.float64) - y[k]).max()))


def _oracle(model, U, V, b, uid, pid, nid, censor=False, bias=True, opt="sgd"):
    from oracle import numpy_oracle as orc
    U, V, b = U.copy(), V.copy(), b.copy()
    oo = orc.SGD(lr=LR) if opt == "sgd" else orc.Adagrad(lr=LR, initial_accumulator_value=0.1, epsilon=1e-7)
    for k in range(uid.shape[0]):
        if not bias:
            b[:] = 0            # (bias-free BPR: the biased step on a bias table that is zero whenever a step starts)
        if model == "bpr":
            orc.bpr_step(U, V, b, uid[k], pid[k], nid[k], oo)
        else:
            orc.ucml_step(U, V, b, uid[k], pid[k], nid[k], oo, margin=0.5, do_censor=censor)
    return dict(U=U, V=V, b=b if bias else None)


def _vs_oracle(got, want, orig, K, what):
    for k in ("U", "V", "b"):
        if got[k] is not None:
            assert np.abs(got[k] - want[k]).max() <= TOL * np.abs(want[k]).max(), (what, k)
            delta_check(orig[k], got[k], want[k], steps=K, what="%s %s" % (what, k))


MODELS = {"bpr": dict(model="bpr"), "bpr_nobias": dict(model="bpr", bias=False), "ucml_censor": dict(model="ucml", censor=True)}
COVER = dict(NU=20000, NI=20000, B=2048, K=3)      # the role-coverage shape


def _assert_roles(uid, pid, nid, NU, NI, B, res, many):
    r = _roles(uid, pid, nid, NU, NI)
    assert r["unique"] > 0 and r["urgent"] > 0, r
    assert (r["many"] > 0) == many, r
    assert 0 < res["pairs"] < r["twice"], "paired rows and refused twice-referenced rows: %d pairs of %d" % (res["pairs"], r["twice"])
    assert 0 < res["max_dup"] * 5 <= B, "the in-launch apply must stay on: %d duplicated rows left of B = %d" % (res["max_dup"], B)


def _agree(runs, ids, orig, K, what, **okw):
    """every run against the oracle (TOL on the tables, delta_check on the updates); bit for bit among themselves where no row has
    three references in a step (otherwise the number of differing elements is printed: a measurement, not a check)"""
    uid, pid, nid = ids
    want = _oracle(okw.pop("model", "bpr"), orig["U"], orig["V"], orig["b"], uid, pid, nid, **okw)
    many = _roles(uid, pid, nid, orig["U"].shape[0], orig["V"].shape[0])["many"]
    for r in runs[1:]:
        if many == 0:
            _same_tables(runs[0], r, what)
        else:
            print("%s: %d rows with >= 3 references; elements that differ: %s" % (
                what, many, {k: int((runs[0][k] != r[k]).sum()) for k in ("U", "V", "b") if r[k] is not None}))
    for r in runs:
        _vs_oracle(r, want, orig, K, what)


# ---- case 1: the same tables with and without the loss
@pytest.mark.parametrize("ids", ["drawn", "thinned"])
@pytest.mark.parametrize("mk", list(MODELS))
@pytest.mark.parametrize("D", [16, 64, 128])
def test_tables_without_the_loss_equal_tables_with_it(D, mk, ids):
    NU, NI, B, K = (COVER[k] for k in ("NU", "NI", "B", "K"))
    U, V, b, uid, pid, nid = _case(100 + D, NU, NI, B, D, K, thin=ids == "thinned")
    with _env(ORX_PLAN_MIN_LATE=1 if ids == "drawn" else None):
        w = _run(U=U, V=V, b=b, uid=uid, pid=pid, nid=nid, want_loss=True, **MODELS[mk])
        wo = _run(U=U, V=V, b=b, uid=uid, pid=pid, nid=nid, want_loss=False, **MODELS[mk])
    for res in (w, wo):
        _assert_roles(uid, pid, nid, NU, NI, B, res, ids == "drawn")
    assert np.isfinite(w["loss"][0]).all() and (w["loss"][0] > 0).all()
    _agree([w, wo], (uid, pid, nid), dict(U=U, V=V, b=b), K, "with / without loss", **MODELS[mk])


@pytest.mark.parametrize("mk", list(MODELS))
@pytest.mark.parametrize("B,rows", [(1, 64), (5, 64), (67, 64), (67, 300)])
def test_small_batches_without_the_loss(B, rows, mk):
    """less than one lane group, less than one wavefront, a ragged last wavefront; tables of 64 rows (B = 67: most rows are
    referenced several times) and, for B = 67 bit for bit, of 300 rows with thinned ids"""
    U, V, b, uid, pid, nid = _case(7 + B, rows, rows, B, 64, 3, thin=rows > 64)
    with _env(ORX_PLAN_MIN_LATE=1):
        w = _run(U=U, V=V, b=b, uid=uid, pid=pid, nid=nid, want_loss=True, **MODELS[mk])
        wo = _run(U=U, V=V, b=b, uid=uid, pid=pid, nid=nid, want_loss=False, **MODELS[mk])
    if B == 1 or rows > 64:
        assert _roles(uid, pid, nid, rows, rows)["many"] == 0
    _agree([w, wo], (uid, pid, nid), dict(U=U, V=V, b=b), 3, "with / without loss, B = %d" % B, **MODELS[mk])


def test_out_of_range_id_without_the_loss():
    """the triplet with the invalid id is skipped, every other one trains, and the index error is still raised"""
    NU, NI, B, K = (COVER[k] for k in ("NU", "NI", "B", "K"))
    U, V, b, uid, pid, nid = _case(33, NU, NI, B, 64, K, thin=True)
    bad = nid.copy(); bad[1, 17] = NI + 7
    with _env():
        w = _run("bpr", U, V, b, uid, pid, bad, want_loss=True, raises=IndexError)
        wo = _run("bpr", U, V, b, uid, pid, bad, want_loss=False, raises=IndexError)
    _same_tables(w, wo, "invalid id, with / without loss")
    touched = np.zeros(NU, bool); touched[uid.reshape(-1)] = True
    assert np.array_equal(wo["U"][~touched], U[~touched]) and (wo["U"][touched] != U[touched]).any()
    keep = np.ones(B, bool); keep[17] = False
    others = np.setdiff1d(uid[1][keep], [uid[1, 17]])
    assert (wo["U"][others] != U[others]).any(axis=1).all(), "valid triplets of the step with the invalid id did not train"


# ---- case 2: the forms without a loss-free kernel called with NULL loss buffers
@pytest.mark.parametrize("form", ["generic_dim", "adagrad", "weighted"])
def test_forms_left_out_still_train_without_loss_buffers(form):
    """D = 50 (generic kernel), Adagrad and the weighted step keep computing their partials; only the sums over them are not launched.
    Thinned ids: tables bit for bit equal to the call that takes the loss."""
    NU, NI, B, K = (COVER[k] for k in ("NU", "NI", "B", "K"))
    D = 50 if form == "generic_dim" else 64
    U, V, b, uid, pid, nid = _case(55, NU, NI, B, D, K, thin=True)
    kw = dict(opt="adagrad") if form == "adagrad" else {}
    if form == "weighted":
        kw["weights"] = np.random.default_rng(3).uniform(0.5, 2.0, (K, B)).astype(np.float32)
    with _env():
        w = _run("bpr", U, V, b, uid, pid, nid, want_loss=True, **kw)
        wo = _run("bpr", U, V, b, uid, pid, nid, want_loss=False, **kw)
    assert np.isfinite(w["loss"][0]).all() and (w["loss"][0] > 0).all()
    assert not np.array_equal(wo["U"], U) and not np.array_equal(wo["V"], V) and not np.array_equal(wo["b"], b)
    if form == "weighted":
        _same_tables(w, wo, form)           # (the weighted objective has an oracle of its own: tests/test_gpu_weighted.py)
    else:
        _agree([w, wo], (uid, pid, nid), dict(U=U, V=V, b=b), K, form, opt=kw.get("opt", "sgd"))


# ---- the call form without the mid-call read-back
def test_second_call_of_a_shape_without_the_loss_and_without_the_read_back():
    """two calls of one shape in one context, neither takes the loss: the second enqueues every launch without reading its plan's
    counters (staging off, the kernels without the bookkeeping); then a call of another shape, which reads its own back.  All three
    against the oracle."""
    rt = _rt()
    NU, NI, B, K, D = 20000, 20000, 2048, 3, 64
    U, V, b, uid, pid, nid = _case(17, NU, NI, B, D, 2 * K)
    B2 = 1500
    _, _, _, uid2, pid2, nid2 = _case(18, NU, NI, B2, D, K)
    f = lambda a: a.reshape(-1)
    with _env():
        ctx = rt.Context(0)
        tU, tV, tb = (rt.Table(*x.shape, ctx).write(x) for x in (U, V, b))
        o = rt.Optimizer.sgd(LR, ctx=ctx)
        assert rt.pairwise_step("bpr", o, tU, tV, tb, f(uid[:K]), f(pid[:K]), f(nid[:K]), K=K, B=B, want_loss=False) is None
        assert ctx.stat("quiet") == 1 and ctx.stat("nowait_calls") == 0
        assert 0 < ctx.stat("max_dup") * 5 <= B and ctx.stat("pairs") > 0
        rt.pairwise_step("bpr", o, tU, tV, tb, f(uid[K:]), f(pid[K:]), f(nid[K:]), K=K, B=B, want_loss=False)
        assert ctx.stat("nowait_calls") == 1
        got1 = dict(U=tU.read(), V=tV.read(), b=tb.read())
        rt.pairwise_step("bpr", o, tU, tV, tb, f(uid2), f(pid2), f(nid2), K=K, B=B2, want_loss=False)
        assert ctx.stat("nowait_calls") == 1, "a call of another shape must read its counters back"
        got2 = dict(U=tU.read(), V=tV.read(), b=tb.read())
        loss, _ = rt.pairwise_step("bpr", o, tU, tV, tb, f(uid2), f(pid2), f(nid2), K=K, B=B2)      # (and the loss is there when asked for again)
    from oracle import numpy_oracle as orc
    Uo, Vo, bo, oo = got2["U"].copy(), got2["V"].copy(), got2["b"].copy(), orc.SGD(lr=LR)
    for k in range(K):
        lw, _ = orc.bpr_step(Uo, Vo, bo, uid2[k], pid2[k], nid2[k], oo)
        assert abs(loss[k] - lw) <= TOL * abs(lw), (k, loss[k], lw)
    want1 = _oracle("bpr", U, V, b, uid, pid, nid)
    _vs_oracle(got1, want1, dict(U=U, V=V, b=b), 2 * K, "two calls of one shape")
    want2 = _oracle("bpr", got1["U"], got1["V"], got1["b"], uid2, pid2, nid2)      # (from the tables the device had then)
    _vs_oracle(got2, want2, got1, K, "then another shape")
