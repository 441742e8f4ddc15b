"""CPU side of the hard-negative sampler: the NumPy restatement of the candidate stream (tests/hardneg_ref.py), which the
GPU test holds the kernel to bit for bit, obeys the sampler's law -- candidates are never positives of the user, uniform over
the rest, independent of M -- and the selection rule on given fp32 scores."""
import numpy as np

import hardneg_ref as hr

NU, NI, NR = 500, 300, 7001


def _z_uniform(users, cand, raw):
    """one-sample chi-square of the candidates against the uniform law over each user's non-positive items, as
    sampler_stats.check_against_golden does it: z = (chi2 - df) / sqrt(2 df)"""
    mult = np.zeros((NU, NI), np.int64); np.add.at(mult, (raw["user_id"], raw["item_id"]), 1)
    cnt = np.zeros((NU, NI), np.int64)
    np.add.at(cnt, (np.repeat(users, cand.shape[1]), cand.reshape(-1)), 1)
    assert (cnt[mult > 0] == 0).all()
    chi2 = df = 0.0
    for u in np.unique(users):
        free = mult[u] == 0
        tot = cnt[u].sum()
        exp = tot / free.sum()
        chi2 += ((cnt[u, free] - exp) ** 2 / exp).sum()
        df += free.sum() - 1
    return (chi2 - df) / np.sqrt(2 * df)


def test_mix64_is_splitmix64_and_the_feistel_walk_is_a_permutation():
    assert int(hr.mix64(0)) == 0xE220A8397B1DCDAF               # the first output of splitmix64 from state 0
    for n, h in ((NR, 7), (1, 1), (16, 2), (17, 3)):
        x = hr.feistel_perm(np.arange(n), n, h, 0x1234567)
        assert np.array_equal(np.sort(x), np.arange(n))


def test_records_are_a_permutation_per_epoch():
    raw = hr.make_data()
    u, p = hr.records(raw, 7, np.arange(2 * NR))
    key = np.sort(raw["user_id"].astype(np.int64) * NI + raw["item_id"])
    for e in range(2):
        sl = slice(e * NR, (e + 1) * NR)
        assert np.array_equal(np.sort(u[sl].astype(np.int64) * NI + p[sl]), key)
    assert not np.array_equal(u[:NR], u[NR:])


def test_candidates_are_never_positives_and_uniform_over_the_rest():
    raw = hr.make_data()
    keys = set(hr.positive_keys(raw, NI).tolist())
    g = np.arange(3 * NR)
    u, p, cand = hr.candidates(raw, NI, 7, g, 8)
    assert cand.min() >= 0 and cand.max() < NI
    assert not any((int(a) * NI + int(c)) in keys for a, row in zip(u, cand) for c in row)
    for cols in (slice(0, 1), slice(5, 6), slice(0, 8)):          # the pairwise sampler's column, a keyed column, all of them
        z = _z_uniform(u, cand[:, cols], raw)
        assert abs(z) < 4.0, (cols, z)
    # the user with 20 % of the items positive: the rejection loop does not tilt the rest
    users = np.full(20000, 3, np.int32)
    _, _, c3 = hr.candidates(raw, NI, 11, np.arange(20000), 4, users=users)
    assert c3.min() >= 60
    z = _z_uniform(users, c3, raw)
    assert abs(z) < 4.0, z
    # columns are different draws
    assert (cand[:, 0] != cand[:, 1]).mean() > 0.9


def test_candidate_c_does_not_depend_on_M_or_on_the_window():
    raw = hr.make_data()
    g = np.arange(6000, 9001)
    _, _, c3 = hr.candidates(raw, NI, 7, g, 3)
    _, _, c8 = hr.candidates(raw, NI, 7, g, 8)
    _, _, c64 = hr.candidates(raw, NI, 7, g, 64)
    assert np.array_equal(c8[:, :3], c3) and np.array_equal(c64[:, :8], c8)
    _, _, w = hr.candidates(raw, NI, 7, g[1000:1500], 8)
    assert np.array_equal(w, c8[1000:1500])
    _, _, other = hr.candidates(raw, NI, 8, g, 3)
    assert not np.array_equal(other, c3)


def _select_loop(row):
    best, sb = 0, row[0]
    for c in range(1, len(row)):
        x = row[c]
        if (not np.isnan(x)) and (np.isnan(sb) or x > sb):
            best, sb = c, x
    return best


def test_selection_rule():
    nan, inf = np.float32("nan"), np.float32("inf")
    rows = np.array([[1, 3, 2, 3], [nan, nan, nan, nan], [nan, -inf, nan, -inf], [-inf, nan, -inf, 0], [nan, 2, 5, nan],
                     [inf, inf, nan, 1], [-inf, -inf, -inf, -inf], [0.0, -0.0, 0, 0], [5, nan, nan, nan]], np.float32)
    assert hr.select(rows).tolist() == [1, 0, 1, 3, 2, 0, 0, 0, 0]
    rng = np.random.default_rng(0)
    s = rng.integers(-3, 4, (2000, 6)).astype(np.float32)            # many ties
    s[rng.random(s.shape) < 0.2] = nan
    s[rng.random(s.shape) < 0.1] = -inf
    assert hr.select(s).tolist() == [_select_loop(r) for r in s]
