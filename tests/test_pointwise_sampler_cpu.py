"""CPU, no library: properties of tests/pointwise_sampler_ref.py itself, so that holding the device's pointwise producers to it bit
for bit (tests/test_gpu_sampler.py) is not a tautology -- and the conditions on the inputs that make that comparison reach the
re-draw and the skip paths."""
import numpy as np
import pytest

import hardneg_ref as hr
import pointwise_sampler_ref as pr
from pointwise_sampler_ref import DENSE, SPARSE

STRAT_SEED, STRAT_N, STRAT_RATIO = 11, 3001, 0.5
PERPOS_SEED, PERPOS_FIRST, PERPOS_N, PERPOS_RATIO = 12, 2000, 3001, 0.2


@pytest.mark.parametrize("shape", [SPARSE, DENSE])
def test_stratified_heads_are_epochs_of_the_records_and_no_tail_is_a_positive(shape):
    raw, NU, NI = pr.data(shape)
    R = len(raw)
    u, i, lab, attempts = pr.stratified(raw, NU, NI, STRAT_SEED, STRAT_N, STRAT_RATIO)
    head = lab == 1.0
    assert set(np.unique(lab)) == {0.0, 1.0} and abs(head.mean() - STRAT_RATIO) < 4 * 0.5 / np.sqrt(STRAT_N)
    key = u.astype(np.int64) * NI + i
    hk = key[head]
    assert len(hk) > 2 * R                                           # the heads cross two epoch boundaries
    rec_key = np.sort(raw["user_id"].astype(np.int64) * NI + raw["item_id"])
    for e in range(len(hk) // R):
        assert np.array_equal(np.sort(hk[e * R:(e + 1) * R]), rec_key)
    assert not np.array_equal(hk[:R], hk[R:2 * R])
    assert not np.isin(key[~head], hr.positive_keys(raw, NI)).any()
    assert (u >= 0).all() and (u < NU).all() and (i >= 0).all() and (i < NI).all()
    assert (attempts[head] == 0).all() and (attempts[~head] >= 1).all() and attempts.max() < 256
    if shape == DENSE:
        assert (attempts[~head] > 1).mean() >= 0.1                   # the re-draw path is taken


@pytest.mark.parametrize("shape", [SPARSE, DENSE])
def test_per_pos_groups_are_a_record_and_distinct_other_items(shape):
    raw, NU, NI = pr.data(shape)
    nneg = pr.per_pos_nneg(PERPOS_RATIO)
    grp = nneg + 1
    assert grp == 5
    q0, q1 = PERPOS_FIRST // grp, (PERPOS_FIRST + PERPOS_N + grp - 1) // grp
    assert q0 < len(raw) < q1                                        # the window crosses the epoch boundary
    g = np.arange(q0 * grp, q1 * grp)                                # whole groups around the window
    u, i, lab, skipped = pr.per_pos(raw, NI, PERPOS_SEED, g, PERPOS_RATIO)
    U, I, L = u.reshape(-1, grp), i.reshape(-1, grp), lab.reshape(-1, grp)
    ru, rp = hr.records(raw, PERPOS_SEED, np.arange(q0, q1))
    assert np.array_equal(U, np.repeat(ru[:, None], grp, 1)) and np.array_equal(I[:, 0], rp)
    assert (L[:, 0] == 1.0).all() and (L[:, 1:] == 0.0).all()
    assert (I[:, 1:] != I[:, :1]).all() and (I >= 0).all() and (I < NI).all()
    assert all(np.unique(row).size == grp for row in I)
    if shape == DENSE:
        w = slice(PERPOS_FIRST - q0 * grp, PERPOS_FIRST - q0 * grp + PERPOS_N)
        assert skipped[w].any()                                      # the skip path is taken inside the window


def test_coin_uses_24_bits_in_float32():
    g = np.arange(4096)
    assert pr.coins(3, g, 1.0).all() and pr.coins(3, g, 0.0).sum() <= 1
    assert 0.2 < pr.coins(3, g, 0.25).mean() < 0.3
