"""CPU side of WARP negative sampling: the resolution rule of tests/warp_ref.py on handwritten rows, `rt.warp_weights` against its
formulas evaluated directly, and the law of the trial count on the pinned candidate stream (tests/hardneg_ref.py)."""
import math

import numpy as np
import pytest

import hardneg_ref as hr
import warp_ref as wr

NU, NI, NR = 500, 300, 7001
INF, NAN = np.float32(np.inf), np.float32(np.nan)


def test_resolve_on_handwritten_rows():
    table = np.array([8.0, 4.0, 2.0, 1.0], np.float32)
    one = np.float32(1.0)
    tie = np.float32(0.75)                       # 0.75 + 0.25 == 1.0 exactly
    rows = [
        # s_p, candidates, margin, t
        (one, [0.0, 0.5, 2.0, 3.0], 0.0, 3),                    # the first violator, not the largest
        (one, [0.0, 0.0, 0.0, 1.5], 0.0, 4),                    # a violator only in the last column
        (one, [0.0, 0.0, 0.0, 0.0], 0.0, 0),                    # none
        (one, [tie, 0.8, 0.0, 0.0], 0.25, 2),                   # s_c + margin == s_p is no violation
        (one, [NAN, 2.0, 0.0, 0.0], 0.0, 2),                    # a NaN candidate never violates
        (one, [NAN, NAN, NAN, NAN], 0.0, 0),
        (NAN, [5.0, INF, 0.0, 0.0], 0.0, 0),                    # a NaN positive: nothing violates
        (NAN, [5.0, INF, 0.0, 0.0], np.inf, 0),
        (one, [-5.0, INF, 0.0, 0.0], 0.0, 2),                   # +inf scores
        (INF, [0.0, INF, 0.0, 0.0], 0.0, 0),                    # inf > inf is false
        (INF, [0.0, INF, 0.0, 0.0], np.inf, 0),
        (one, [-7.0, 0.0, 0.0, 0.0], np.inf, 1),                # margin = +inf: the first finite candidate
        (one, [-INF, 3.0, 0.0, 0.0], np.inf, 2),                # -inf + inf is NaN
        (one, [9.0, INF, 0.0, 0.0], -np.inf, 0),                # margin = -inf: nothing (inf - inf is NaN)
        (-INF, [0.0, 0.0, 0.0, 0.0], -np.inf, 0),               # -inf > -inf is false
    ]
    sp = np.array([r[0] for r in rows], np.float32)
    sc = np.array([r[1] for r in rows], np.float32)
    for i, (_, _, margin, want) in enumerate(rows):
        t, col, w = wr.resolve(sp[i:i + 1], sc[i:i + 1], margin, table)
        assert t[0] == want, (i, t[0], want)
        assert col[0] == max(want - 1, 0)
        assert w.dtype == np.float32 and w.view(np.int32)[0] == (table[want - 1].view(np.int32) if want else 0), i
    # many rows at once, one margin
    t, col, w = wr.resolve(sp[:3], sc[:3], 0.0, table)
    assert t.tolist() == [3, 4, 0] and col.tolist() == [2, 3, 0] and w.tolist() == [2.0, 1.0, 0.0]
    # the add is rounded to fp32 before the compare: 1 + 2^-25 is 1 in fp32, no violation of s_p = 1
    t, _, _ = wr.resolve([one], [[one]], 2.0 ** -25, table[:1])
    assert t[0] == 0


def _direct(total_items, T, kind):
    out = []
    for t in range(1, T + 1):
        r = (total_items - 1) // t
        if kind == "log":
            out.append(math.log(max(1, r)))
        elif kind == "log1p":
            out.append(math.log(r + 1))
        else:
            out.append(math.fsum(1.0 / np.arange(1, r + 1, dtype=np.float64)))
    return np.array(out, np.float64)


@pytest.mark.parametrize("kind", ["log", "log1p", "harmonic"])
def test_warp_weights_are_their_formulas(kind):
    """float64 then one cast: an fp64 evaluation is within n 2^-53 relative of the exact value, far inside half an fp32 ulp, so
    the cast of any correct fp64 evaluation is within ONE fp32 ulp of the cast of the direct one (equal unless the value sits on
    a rounding boundary)"""
    from openrec_amd import runtime as rt
    for items in (2, 300, 1_000_000):
        for T in (1, 10, 256):
            want = _direct(items, T, kind)
            got = rt.warp_weights(items, T, kind)
            assert got.shape == (T,) and got.dtype == np.float32
            w32 = want.astype(np.float32)
            assert (np.abs(got.astype(np.float64) - w32) <= np.spacing(np.abs(w32))).all(), (items, T)
            assert (got >= 0).all() and (np.diff(got) <= 0).all()                # a smaller rank estimate never weighs more
    assert np.array_equal(rt.warp_weights(300, 10), rt.warp_weights(300, 10, "log"))
    # r_t = floor(299 / t): t = 1 -> 299, t = 150 -> 1, t = 256 -> 1 (300 items); with 2 items r_1 = 1, r_t = 0 beyond
    w = rt.warp_weights(2, 3, kind)
    assert w[1] == 0 and w[2] == 0 and (w[0] == 0) == (kind == "log")


def test_warp_weights_normalize_and_errors():
    from openrec_amd import runtime as rt
    for kind in ("log", "log1p", "harmonic"):
        w, wn = rt.warp_weights(300, 16, kind), rt.warp_weights(300, 16, kind, normalize=True)
        assert wn[0] == 1.0 and wn.dtype == np.float32
        want = (_direct(300, 16, kind) / _direct(300, 16, kind)[0]).astype(np.float32)
        assert (np.abs(wn - want) <= np.spacing(want)).all()
        assert np.allclose(wn * w[0], w, rtol=1e-6)
    for bad in (dict(total_items=1), dict(total_items=0), dict(max_trials=0), dict(max_trials=257), dict(kind="exp"),
                dict(kind=None)):
        kw = dict(total_items=300, max_trials=10, kind="log"); kw.update(bad)
        with pytest.raises(ValueError):
            rt.warp_weights(**kw)


@pytest.mark.parametrize("seed,k,T", [(7, 30, 16), (11, 60, 16), (7, 10, 64)])
def test_the_trial_count_is_geometric_on_the_pinned_stream(seed, k, T):
    """"violates" := item id >= NI - k.  Candidates are independent and uniform over the user's non-positives, so t is geometric
    with q_u = (non-positive violators of u) / (non-positives of u): P(t = j) = (1 - q)^(j - 1) q, P(t = 0) = (1 - q)^T.  Pooled
    over the samples, bins of expectation >= 5 (the others pooled into one), z = (chi2 - df) / sqrt(2 df), |z| < 4."""
    raw = hr.make_data()
    g = np.arange(3 * NR)
    u, p, cand = hr.candidates(raw, NI, seed, g, T)
    viol = cand >= NI - k
    # resolve() on scores that encode the event: s_p = 0, s_c = +-1, margin 0
    t, col, _ = wr.resolve(np.zeros(len(g), np.float32), np.where(viol, 1.0, -1.0).astype(np.float32), 0.0, np.ones(T, np.float32))
    assert np.array_equal(t > 0, viol.any(1)) and (viol[np.arange(len(g)), col] == (t > 0)).all()
    pos = np.zeros((NU, NI), bool); pos[raw["user_id"], raw["item_id"]] = True
    free = (~pos).sum(1).astype(np.float64)
    q = (~pos[:, NI - k:]).sum(1) / free
    qs = q[u]
    exp = np.zeros(T + 1)
    exp[0] = ((1 - qs) ** T).sum()
    for j in range(1, T + 1):
        exp[j] = ((1 - qs) ** (j - 1) * qs).sum()
    assert abs(exp.sum() - len(g)) < 1e-6
    obs = np.bincount(t, minlength=T + 1).astype(np.float64)
    big = exp >= 5
    o, e = list(obs[big]), list(exp[big])
    if (~big).any() and exp[~big].sum() >= 5:
        o.append(obs[~big].sum()); e.append(exp[~big].sum())
    o, e = np.array(o), np.array(e)
    df = len(e) - 1
    assert df >= 5
    z = (((o - e) ** 2 / e).sum() - df) / np.sqrt(2 * df)
    print(f"seed {seed} k {k} T {T}: {len(e)} bins, z = {z:.2f}, mean t {t[t > 0].mean():.2f}, none {np.mean(t == 0):.3f}")
    assert abs(z) < 4, z
