"""Candidate lists without a device: the three entry points are exported and typed, the host-only list check, and
`Dataset.evaluation(candidates=True)`, whose `cand_mask` is exactly the complement of the default mode's dense `excl_mask`."""
import ctypes

import numpy as np
import pytest

NAMES = ("orx_score_candidates", "orx_rank_metrics_candidates", "orx_rank_metrics_candidates_check")


def test_entry_points_are_exported_and_typed():
    from openrec_amd import _ffi
    lib = _ffi.load()
    for name in NAMES:
        assert name in _ffi.SIGNATURES, name
        fn = getattr(lib, name)
        res, args = _ffi.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert len(_ffi.SIGNATURES["orx_score_candidates"][1]) == 12
    assert len(_ffi.SIGNATURES["orx_rank_metrics_candidates"][1]) == 18
    assert _ffi.SIGNATURES["orx_rank_metrics_candidates"][1][14] is ctypes.c_size_t


def _masks(rt, pos, cand, NI):
    return rt.SparseMask.from_lists(pos, NI), rt.SparseMask.from_lists(cand, NI)


def test_check_returns_the_longest_lists():
    from openrec_amd import runtime as rt
    NI = 50
    pos, cand = _masks(rt, [[1, 2, 3], [], [49]], [[0, 1, 2, 3, 9], [4], list(range(50))], NI)
    assert rt.rank_metrics_candidates_check(pos, cand) == (3, 50)
    empty = rt.SparseMask(np.zeros(1, np.int64), np.zeros(0, np.int32), NI)
    assert rt.rank_metrics_candidates_check(empty, empty) == (0, 0)


@pytest.mark.parametrize("which", ["positive", "candidate"])
@pytest.mark.parametrize("row", [[5, 3, 7], [3, 3, 7]], ids=["unsorted", "repeated"])
def test_check_names_user_and_list_of_a_bad_row(which, row):
    from openrec_amd import runtime as rt
    NI = 50
    good = rt.SparseMask.from_lists([[1, 2], [4, 5, 6], [7]], NI)
    bad = rt.SparseMask(np.array([0, 2, 5, 6], np.int64), np.array([1, 2] + row + [7], np.int32), NI)
    pos, cand = (bad, good) if which == "positive" else (good, bad)
    with pytest.raises(ValueError) as e:
        rt.rank_metrics_candidates_check(pos, cand)
    assert f"{which} list of user 1" in str(e.value)


@pytest.mark.parametrize("which", ["positive", "candidate"])
@pytest.mark.parametrize("bad_id", [-1, 50])
def test_check_raises_index_error_outside_the_table(which, bad_id):
    from openrec_amd import runtime as rt
    NI = 50
    good = rt.SparseMask.from_lists([[1, 2], [4, 5, 6]], NI)
    items = np.array([1, 2, 4, 5, 6], np.int32)
    items[0 if bad_id < 0 else 4] = bad_id
    bad = rt.SparseMask(np.array([0, 2, 5], np.int64), items, NI)
    pos, cand = (bad, good) if which == "positive" else (good, bad)
    with pytest.raises(IndexError):
        rt.rank_metrics_candidates_check(pos, cand)


def test_candidate_lists_keep_order_and_repeats():
    from openrec_amd import runtime as rt
    c = rt.CandidateLists.from_lists([[9, 3, 3, 0], [], [7]], 10)
    assert c.shape == (3, 10) and c.ptr.tolist() == [0, 4, 4, 5] and c.items.tolist() == [9, 3, 3, 0, 7]
    assert c.items.dtype == np.int32 and c.row(0).tolist() == [9, 3, 3, 0]
    with pytest.raises(IndexError):
        rt.CandidateLists.from_lists([[10]], 10)
    m = rt.SparseMask.from_lists([[1]], 10)
    assert rt.as_candidate_lists(m, 10) is m and rt.as_candidate_lists([[2, 1]], 10).items.tolist() == [2, 1]


def _raw(rng, n, NU, NI):
    a = np.zeros(n, dtype=[("user_id", np.int32), ("item_id", np.int32)])
    a["user_id"] = rng.integers(0, NU, n); a["item_id"] = rng.integers(0, NI, n)
    return a


def test_dataset_candidates_are_the_complement_of_the_dense_exclusions():
    from openrec_amd import runtime as rt
    from openrec_amd.tf2.data import Dataset
    rng = np.random.default_rng(3)
    NU, NI = 60, 200
    np.random.seed(7)
    train = Dataset(_raw(rng, 900, NU, NI), NU, NI, seed=1)
    val = Dataset(_raw(rng, 300, NU, NI), NU, NI, num_negatives=5, seed=1)
    dense = list(val.evaluation(16, [train]))
    cands = list(val.evaluation(16, [train], candidates=True))
    assert len(dense) == len(cands) > 1
    for d, c in zip(dense, cands):
        assert set(c) == {"user_id", "pos_mask", "cand_mask"}
        assert isinstance(c["cand_mask"], rt.SparseMask) and isinstance(c["pos_mask"], rt.SparseMask)
        assert np.array_equal(c["user_id"], d["user_id"])
        assert np.array_equal(np.asarray(c["cand_mask"]), ~np.asarray(d["excl_mask"]))
        assert np.array_equal(np.asarray(c["pos_mask"]), np.asarray(d["pos_mask"]))
        rt.rank_metrics_candidates_check(c["pos_mask"], c["cand_mask"])          # strictly ascending rows
    # without excl_datasets the candidates are the positives and the sampled negatives
    c = next(iter(val.evaluation(16, candidates=True)))
    d = next(iter(val.evaluation(16)))
    assert np.array_equal(np.asarray(c["cand_mask"]), ~np.asarray(d["excl_mask"]))


def test_dataset_candidates_need_explicit_negatives():
    from openrec_amd.tf2.data import Dataset
    rng = np.random.default_rng(4)
    implicit = Dataset(_raw(rng, 100, 20, 30), 20, 30, seed=1)
    with pytest.raises(ValueError):
        implicit.evaluation(8, candidates=True)
    assert set(next(iter(implicit.evaluation(8)))) == {"user_id", "pos_mask", "excl_mask"}     # the default is unchanged


def test_evaluate_refuses_both_masks():
    from openrec_amd.tf2.recommenders._base import Recommender
    m = object.__new__(Recommender)
    with pytest.raises(ValueError):
        Recommender.evaluate(m, np.zeros(1, np.int32), None, excl_mask=np.zeros((1, 3), bool), cand_mask=np.zeros((1, 3), bool))
