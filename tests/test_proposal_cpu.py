"""CPU side of the weighted item proposal: the host-only alias-table builder (orx_alias_build) reproduces its weights to the
32-bit quantisation and never yields an item of weight 0; the NumPy restatement of the draw (tests/proposal_ref.py), which the
GPU test holds the kernels to bit for bit, obeys the proposal and keeps the give-up rule of the uniform draw."""
import ctypes

import numpy as np
import pytest

import hardneg_ref as hr
import proposal_ref as pr

NU, NI, NR = 500, 300, 7001


def _build(w):
    from openrec_amd import runtime as rt
    return rt.alias_build(w)


def _popularity(alpha=0.75):
    raw = hr.make_data()
    keys = hr.positive_keys(raw, NI)
    return np.bincount(keys % NI, minlength=NI).astype(np.float64) ** alpha      # distinct users per item


def _cases():
    rng = np.random.default_rng(5)
    z = np.zeros(300); z[rng.permutation(300)[:50]] = rng.random(50) + 0.01
    zipf = (1.0 / np.arange(1, 4100) ** 1.05)[rng.permutation(4099)]
    heavy = np.full(1000, 0.001 / 999); heavy[17] = 0.999
    return {"one": np.array([2.5]), "two": np.array([1.0, 3.0]), "popularity": _popularity(), "zeros250": z, "zipf4099": zipf,
            "heavy": heavy, "random2p20": rng.random(1 << 20)}


CASES = _cases()


@pytest.mark.parametrize("name", list(CASES))
def test_table_is_exact(name):
    """|q_i - w_i / sum(w)| <= 2^-30 with q the probability the table implies: the quantisation of the thresholds is at most
    2^-32 in total over the columns that alias to i, Vose's rounding at most n 2^-52 <= 2^-32 for n <= 2^20: a factor two of
    margin.  q_i == 0 exactly wherever w_i == 0."""
    w = CASES[name]
    n = len(w)
    thr, alias = _build(w)
    assert thr.dtype == np.uint32 and alias.dtype == np.int32 and len(thr) == n and len(alias) == n
    assert alias.min() >= 0 and alias.max() < n
    q = pr.implied_probabilities(thr, alias)
    assert int(q.sum()) == n << 32
    err = np.abs(q / float(n << 32) - w / w.sum())
    print(f"{name}: n = {n}, max |q - w / sum w| = {err.max():.3g} = {err.max() * 2.0 ** 30:.3g} x 2^-30")
    assert err.max() <= 2.0 ** -30
    zero = w == 0
    assert (q[zero] == 0).all()
    assert (thr[zero] == 0).all() and not np.isin(alias, np.nonzero(zero)[0]).any()     # own column never, and nobody's alias
    if name == "two":
        assert q.tolist() == [1 << 31, 3 << 31]           # (1/4, 3/4) exactly


def test_equal_weights_keep_every_column_whole():
    for n in (1, 2, 300, 4099):
        thr, alias = _build(np.ones(n))
        assert np.array_equal(alias, np.arange(n))


def test_bad_weights_are_refused_and_nothing_is_written():
    from openrec_amd import _ffi, runtime as rt
    lib = _ffi.load()
    nan, inf = float("nan"), float("inf")
    bad = [([], 0), ([1.0], -3), ([1.0, 2.0], (1 << 31)), ([1.0, nan, 2.0], 3), ([1.0, inf], 2), ([1.0, -inf], 2),
           ([3.0, -1e-300, 2.0], 3), ([0.0, 0.0, 0.0], 3), ([0.0], 1), ([1.0, 2.0, nan], 3)]
    for vals, n in bad:
        w = np.array(vals + [1.0], np.float64)            # (never an empty buffer)
        thr = np.full(8, 0xDEADBEEF, np.uint32); alias = np.full(8, -77, np.int32)
        rc = lib.orx_alias_build(w.ctypes.data, ctypes.c_int64(n), thr.ctypes.data, alias.ctypes.data)
        assert rc == _ffi.ORX_ERR_ARG, (vals, n)
        assert (thr == 0xDEADBEEF).all() and (alias == -77).all(), (vals, n)
    for vals in ([], [nan], [1.0, -1.0], [0.0, 0.0], [inf, 1.0]):
        with pytest.raises(ValueError):
            rt.alias_build(np.array(vals, np.float64))
    thr, alias = rt.alias_build([0.0, 5.0])               # the call still works afterwards; the whole mass on item 1
    assert pr.implied_probabilities(thr, alias).tolist() == [0, 2 << 32]


def _chi2_critical(df, z):
    """Wilson-Hilferty: the chi-square quantile of the standard normal quantile z; at df > 100 it is within 0.1 of the exact value"""
    return df * (1 - 2 / (9 * df) + z * np.sqrt(2 / (9 * df))) ** 3


def test_the_reference_stream_obeys_the_proposal():
    """User 3 (60 positives among the items 0..79 that hold half the mass, so the rejection loop works hard): its candidates
    against w restricted to its non-positives and renormalised, chi-square at the 1e-4 level (z = 3.719).  2500 samples x 8
    candidates = 20000 draws; the lightest cell has probability (0.5 / 210) / 0.625 = 1 / 262.5 or more: >= 76 expected."""
    raw = hr.make_data()
    w = np.zeros(NI)
    w[:80] = 0.5 / 80; w[80:290] = 0.5 / 210             # items 290..299: weight 0
    thr, alias = _build(w)
    n, M = 2500, 8
    users = np.full(n, 3, np.int32)
    _, _, cand = pr.candidates(raw, NI, 11, np.arange(n), M, thr, alias, users=users)
    pos = np.zeros(NI, bool); pos[raw["item_id"][raw["user_id"] == 3]] = True
    assert pos[:60].all()
    cnt = np.bincount(cand.reshape(-1), minlength=NI)
    assert cnt[pos].sum() == 0 and cnt[w == 0].sum() == 0
    cell = ~pos & (w > 0)
    exp = w[cell] / w[cell].sum() * cnt.sum()
    assert exp.min() >= 20
    chi2 = float(((cnt[cell] - exp) ** 2 / exp).sum())
    df = int(cell.sum()) - 1
    crit = _chi2_critical(df, 3.719)
    print(f"chi2 = {chi2:.1f}, df = {df}, critical value at 1e-4 = {crit:.1f}, least expected count = {exp.min():.1f}")
    assert chi2 < crit
    # every candidate column on its own draws from the proposal too: the heavy items 60..79 come up about 0.2 of the time
    heavy = w[cell & (np.arange(NI) < 80)].sum() / w[cell].sum()
    for c in (0, 5):
        share = (cand[:, c] < 80).mean()
        assert abs(share - heavy) < 4 * np.sqrt(heavy * (1 - heavy) / n), (c, share, heavy)
    # and the uniform stream is another one
    _, _, unif = hr.candidates(raw, NI, 11, np.arange(n), M, users=users)
    assert not np.array_equal(unif, cand)


def test_all_ones_is_the_uniform_stream():
    raw = hr.make_data()
    thr, alias = _build(np.ones(NI))
    g = np.arange(6000, 8000)
    a = pr.candidates(raw, NI, 7, g, 8, thr, alias)
    b = hr.candidates(raw, NI, 7, g, 8)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_a_user_without_a_free_item_of_positive_weight_keeps_the_last_draw():
    """every item of positive weight is a positive of user 3: all 256 attempts are rejected and attempt 255 stays, as in the
    uniform draw"""
    raw = hr.make_data()
    w = np.zeros(NI); w[:60] = np.arange(1, 61)
    thr, alias = _build(w)
    n, seed = 50, 13
    g = np.arange(100, 100 + n)
    _, _, cand = pr.candidates(raw, NI, seed, g, 1, thr, alias, users=np.full(n, 3, np.int32))
    with np.errstate(over="ignore"):
        r = hr.mix64(hr.U64(seed) ^ (g.astype(hr.U64) * hr.U64(0x9E3779B97F4A7C15)) ^ hr.U64(255 << 56) ^ hr.U64(0xA5A5A5A5))
        j = (r % hr.U64(NI)).astype(np.int64)
        t = (hr.mix64(r ^ hr.U64(0x5851F42D4C957F2D)) >> hr.U64(32)).astype(np.uint32)
    last = np.where(t < thr[j], j, alias[j])
    assert np.array_equal(cand[:, 0], last) and cand.max() < 60 and len(np.unique(cand)) > 10
