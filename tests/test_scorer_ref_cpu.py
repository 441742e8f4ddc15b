"""scorer_ref's checker can fail: correct fp32 evaluations of the scorer's arithmetic pass `check` and `check_exact`, and every
mutant a kernel could plausibly be -- a dropped column, unzeroed padding, a shifted bias, swapped items, a misplaced row, an
unwritten element, lost precision, a wrong sign in the expanded L2 form -- is rejected.  No GPU."""
import numpy as np
import pytest

import scorer_ref as sr

NU, NI, NQ = 40, 37, 11
DIMS = (3, 20, 64, 300)


def _uid(rng):
    return rng.integers(0, NU, NQ).astype(np.int32)


def _normal(rng, D):
    U = rng.normal(size=(NU, D)).astype(np.float32); V = rng.normal(size=(NI, D)).astype(np.float32)
    w = rng.normal(size=(D, 1)).astype(np.float32); b = rng.normal(size=(NI, 1)).astype(np.float32)
    return U, V, w, b


def fp32_scores(kind, U, V, b, w, uid, order="uw", D_used=None, garbage=None, trunc=None, l2_sign=-1.0, bias_shift=0):
    """the scorer in fp32, one rounding per operation, columns accumulated one after the other.
    order      gmf: "uw" (u*w)*v, the matrix-core kernel's; "uv" (u*v)*w, the plain kernel's
    D_used     columns summed (a mutant that drops the tail)
    garbage    two [Dp - D] vectors that stand in the user and the item tile beyond D (a mutant that never zeroed them)
    trunc      mantissa bits kept of every operand
    l2_sign    the sign of |v|^2 in the expanded form, -1 when correct
    bias_shift the bias comes from item j + bias_shift"""
    f = np.float32
    u = U[uid].astype(f); v = V.astype(f); ww = None if w is None else w.reshape(-1).astype(f)
    if trunc is not None:
        def cut(x):
            m = np.int32(-1) << np.int32(23 - trunc)
            return (x.view(np.int32) & m).view(f)
        u, v = cut(np.ascontiguousarray(u)), cut(np.ascontiguousarray(v))
        ww = None if ww is None else cut(np.ascontiguousarray(ww))
    D = u.shape[1] if D_used is None else D_used
    if garbage is not None:
        gu, gv = (np.asarray(g, f) for g in garbage)
        u = np.concatenate([u[:, :D], np.broadcast_to(gu, (u.shape[0], gu.size))], 1)
        v = np.concatenate([v[:, :D], np.broadcast_to(gv, (v.shape[0], gv.size))], 1)
        if ww is not None:
            ww = np.concatenate([ww[:D], np.ones(gu.size, f)])
        D = u.shape[1]
    acc = np.zeros((u.shape[0], v.shape[0]), f)
    un = np.zeros(u.shape[0], f); vn = np.zeros(v.shape[0], f)
    for k in range(D):
        uk, vk = u[:, k], v[:, k]
        if kind == "gmf":
            p = (uk * ww[k])[:, None] * vk[None, :] if order == "uw" else (uk[:, None] * vk[None, :]) * ww[k]
        else:
            p = uk[:, None] * vk[None, :]
        acc = acc + p.astype(f)
        un = un + uk * uk; vn = vn + vk * vk
    if kind == "l2":                                  # the expanded form: 2 u.v - |u|^2 - |v|^2
        acc = (f(2.0) * acc - un[:, None]) + f(l2_sign) * vn[None, :]
    if b is not None:
        acc = acc + np.roll(b.reshape(-1).astype(f), -bias_shift)[None, :]
    assert acc.dtype == f
    return acc


def fp32_direct_l2(U, V, b, uid):
    """-sum (u - v)^2 in fp32, the plain kernel's form"""
    f = np.float32
    u = U[uid]; acc = np.zeros((u.shape[0], V.shape[0]), f)
    for k in range(u.shape[1]):
        d = u[:, k][:, None] - V[:, k][None, :]
        acc = acc - d * d
    return acc if b is None else acc + b.reshape(-1)[None, :]


def _rejected(fn, *a):
    with pytest.raises(AssertionError):
        fn(*a)


@pytest.mark.parametrize("D", DIMS + (1, 7, 256, 1024))
def test_exact_tables_are_exact_in_any_order_and_form(D):
    rng = np.random.default_rng(D)
    U, V, w, b = sr.exact_tables(rng, NU, NI, D)
    assert U.dtype == V.dtype == w.dtype == b.dtype == np.float32
    assert np.abs(U).max() <= 3 and np.abs(V).max() <= 3 and np.abs(w).max() <= 2 and np.abs(b).max() <= 8
    assert w.shape == (D, 1) and b.shape == (NI, 1)
    uid = _uid(rng)
    rev = slice(None, None, -1)
    for bias in (b, None):
        for kind in sr.KINDS:
            for order in ("uw", "uv"):
                sr.check_exact(fp32_scores(kind, U, V, bias, w, uid, order), kind, U, V, bias, w, uid)
            # the columns summed backwards
            sr.check_exact(fp32_scores(kind, U[:, rev], V[:, rev], bias, w[rev], uid), kind, U, V, bias, w, uid)
        sr.check_exact(fp32_direct_l2(U, V, bias, uid), "l2", U, V, bias, w, uid)


@pytest.mark.parametrize("D", DIMS)
def test_correct_fp32_evaluations_stay_inside_the_bound(D):
    rng = np.random.default_rng(100 + D)
    U, V, w, b = _normal(rng, D)
    uid = _uid(rng)
    for bias in (b, None):
        for kind in sr.KINDS:
            for order in ("uw", "uv"):
                sr.check(fp32_scores(kind, U, V, bias, w, uid, order), kind, U, V, bias, w, uid)
        sr.check(fp32_direct_l2(U, V, bias, uid), "l2", U, V, bias, w, uid)


def test_the_reference_is_the_direct_form_in_float64():
    rng = np.random.default_rng(5)
    U, V, w, b = _normal(rng, 9)
    uid = np.array([3, 3, 0, NU - 1], np.int32)
    U64, V64 = U.astype(np.float64), V.astype(np.float64)
    want = np.array([[-((U64[u] - V64[j]) ** 2).sum() + float(b[j, 0]) for j in range(NI)] for u in uid])
    got = sr.reference("l2", U, V, b, None, uid)
    assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-13, atol=0)      # (float64 sums in another order)
    assert np.allclose(sr.reference("gmf", U, V, None, w, uid), (U64[uid] * w[:, 0].astype(np.float64)) @ V64.T, rtol=1e-14, atol=0)
    assert np.allclose(sr.reference("dot", U, V, b, None, uid) - sr.reference("dot", U, V, None, None, uid),
                       np.broadcast_to(b[:, 0].astype(np.float64), (4, NI)), rtol=0, atol=1e-13)


def test_check_holds_shape_dtype_and_finiteness():
    rng = np.random.default_rng(6)
    U, V, w, b = _normal(rng, 20)
    uid = _uid(rng)
    good = fp32_scores("dot", U, V, b, w, uid)
    sr.check(good, "dot", U, V, b, w, uid)
    _rejected(sr.check, good[:-1], "dot", U, V, b, w, uid)
    _rejected(sr.check, good[:, :-1], "dot", U, V, b, w, uid)
    _rejected(sr.check, good.astype(np.float64), "dot", U, V, b, w, uid)
    _rejected(sr.check_exact, good.astype(np.float64), "dot", U, V, b, w, uid)
    for v in (np.nan, np.inf, -np.inf):
        bad = good.copy(); bad[4, 9] = v
        _rejected(sr.check, bad, "dot", U, V, b, w, uid)
    # a non-finite reference element must not come back finite
    Vn = V.copy(); Vn[5] = np.nan
    out = fp32_scores("dot", U, Vn, b, w, uid)
    sr.check(out, "dot", U, Vn, b, w, uid)
    out[2, 5] = 0.0
    _rejected(sr.check, out, "dot", U, Vn, b, w, uid)
    # the failure names the worst elements
    bad = good.copy(); bad[7, 3] += 1.0
    with pytest.raises(AssertionError, match=r"q=7, j=3"):
        sr.check(bad, "dot", U, V, b, w, uid)


def _both_modes(D, seed):
    """(checker, tables) of the exact and of the bounded mode"""
    rng = np.random.default_rng(seed)
    yield sr.check_exact, sr.exact_tables(rng, NU, NI, D), rng
    yield sr.check, _normal(rng, D), rng


@pytest.mark.parametrize("kind", sr.KINDS)
@pytest.mark.parametrize("D", DIMS)
def test_arithmetic_mutants_are_rejected(D, kind):
    for chk, (U, V, w, b), rng in _both_modes(D, 200 + D):
        uid = _uid(rng)
        a = (kind, U, V, b, w, uid)
        chk(fp32_scores(*a), *a)
        # the last column dropped (exact tables: a last column of zeros would hide it, so it is made non-zero first)
        U[:, -1] = np.where(U[:, -1] == 0, 1, U[:, -1]); V[:, -1] = np.where(V[:, -1] == 0, 2, V[:, -1]); w[-1] = 1 if w[-1] == 0 else w[-1]
        chk(fp32_scores(*a), *a)
        _rejected(chk, fp32_scores(*a, D_used=D - 1), *a)
        # columns D .. Dp-1 of the tiles not zeroed
        Dp = 16 * ((D + 15) // 16) if D % 16 else D + 16
        if chk is sr.check_exact:                        # (different in the two tiles: equal garbage cancels in the expanded L2 form)
            gu = rng.integers(1, 4, Dp - D); garbage = (gu, gu + 1)
        else:
            garbage = (rng.normal(size=Dp - D), rng.normal(size=Dp - D))
        _rejected(chk, fp32_scores(*a, garbage=garbage), *a)
        # a single unzeroed column
        _rejected(chk, fp32_scores(*a, garbage=(garbage[0][:1], garbage[1][:1])), *a)
        # the bias of item j + 1
        _rejected(chk, fp32_scores(*a, bias_shift=1), *a)
        if kind == "l2":
            _rejected(chk, fp32_scores(*a, l2_sign=+1.0), *a)
            _rejected(chk, fp32_scores(kind, U, V, None, w, uid, l2_sign=+1.0), kind, U, V, None, w, uid)


@pytest.mark.parametrize("kind", sr.KINDS)
@pytest.mark.parametrize("D", DIMS)
def test_placement_mutants_are_rejected(D, kind):
    for chk, (U, V, w, b), rng in _both_modes(D, 300 + D):
        uid = np.arange(NQ, dtype=np.int32)              # distinct users: no two rows are equal by construction
        a = (kind, U, V, b, w, uid)
        good = fp32_scores(*a)
        chk(good, *a)
        # two adjacent items swapped in one row
        q = 5
        j = int(np.argmax(good[q, :-1] != good[q, 1:]))
        assert good[q, j] != good[q, j + 1]
        bad = good.copy(); bad[q, [j, j + 1]] = bad[q, [j + 1, j]]
        _rejected(chk, bad, *a)
        # one user's row written at q + 1 (row q keeps what the previous call left there)
        stale = fp32_scores(kind, U, V, b, w, (uid + NQ) % NU)
        assert not np.array_equal(good[q], good[q + 1])
        bad = good.copy(); bad[q + 1] = good[q]; bad[q] = stale[q]
        _rejected(chk, bad, *a)
        bad = good.copy(); bad[q + 1] = good[q]          # ... even when row q is written as well
        _rejected(chk, bad, *a)
        # one element left at a stale value: the previous call's, and a zero
        jj = int(np.argmax(stale[q] != good[q]))
        assert stale[q, jj] != good[q, jj]
        bad = good.copy(); bad[q, jj] = stale[q, jj]
        _rejected(chk, bad, *a)
        jz = int(np.argmax(good[NQ - 1] != 0))
        bad = good.copy(); bad[NQ - 1, jz] = 0.0
        _rejected(chk, bad, *a)
        # the last element of the matrix, off by the smallest amount the mode can see
        bad = good.copy()
        bad[-1, -1] += 1.0 if chk is sr.check_exact else 3 * float(sr.bound(*a)[-1, -1]) + float(np.spacing(np.abs(bad[-1, -1])))
        _rejected(chk, bad, *a)


@pytest.mark.parametrize("bits", [10, 7])
@pytest.mark.parametrize("kind", sr.KINDS)
@pytest.mark.parametrize("D", DIMS)
def test_truncated_operands_are_rejected(D, kind, bits):
    """bf16-like (7 bits) and tf32-like (10 bits) operands: what a reduced-precision matrix instruction would give"""
    rng = np.random.default_rng(400 + D)
    U, V, w, b = _normal(rng, D)
    uid = _uid(rng)
    for bias in (b, None):
        a = (kind, U, V, bias, w, uid)
        _rejected(sr.check, fp32_scores(*a, trunc=bits), *a)
    # and most elements violate the bound, not a stray one
    err = np.abs(fp32_scores(kind, U, V, b, w, uid, trunc=bits).astype(np.float64) - sr.reference(kind, U, V, b, w, uid))
    assert (err > sr.bound(kind, U, V, b, w, uid)).mean() > 0.5
