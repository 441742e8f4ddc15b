"""Ranking metrics without a score matrix, the parts that need no device: the entry points are exported and typed, the list
checks made before any device work raise the documented errors, and the scratch query stays within its budget however
large users x items gets."""
import numpy as np
import pytest

from openrec_amd import _ffi
from openrec_amd import runtime as rt

MB = 1 << 20


def test_the_entry_points_are_exported_and_typed():
    lib = _ffi.load()
    for name, nargs in (("orx_rank_metrics_matrixfree", 18), ("orx_rank_metrics_matrixfree_scratch", 9),
                        ("orx_rank_metrics_matrixfree_check", 8)):
        assert hasattr(lib, name)
        assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == nargs
    assert callable(rt.rank_metrics_matrixfree) and callable(rt.rank_metrics_matrixfree_scratch)


def _mask(rows, NI):
    ptr = np.zeros(len(rows) + 1, np.int64); np.cumsum([len(r) for r in rows], out=ptr[1:])
    return rt.SparseMask(ptr, np.concatenate([np.asarray(r, np.int32) for r in rows]).astype(np.int32), NI)


def test_sorted_lists_pass_and_report_the_longest():
    pos = rt.SparseMask.from_lists([[5, 1, 3], [], [7]], 10)
    excl = rt.SparseMask.from_lists([[2], [0, 1, 2, 9], []], 10)
    assert rt.rank_metrics_matrixfree_check(pos, excl) == (3, 4)


def test_an_unsorted_list_is_a_value_error_naming_the_user():
    ok = _mask([[1, 2], [3, 4], []], 10)
    with pytest.raises(ValueError, match="positive list of user 1 .*strictly ascending"):
        rt.rank_metrics_matrixfree_check(_mask([[1, 2], [4, 3], []], 10), ok)
    with pytest.raises(ValueError, match="exclusion list of user 2 .*strictly ascending"):
        rt.rank_metrics_matrixfree_check(ok, _mask([[1], [], [0, 5, 2]], 10))


def test_a_repeated_item_is_a_value_error_naming_the_user():
    ok = _mask([[1, 2], [3, 4], []], 10)
    with pytest.raises(ValueError, match="positive list of user 0 .*strictly ascending"):
        rt.rank_metrics_matrixfree_check(_mask([[1, 2, 2], [3], []], 10), ok)
    with pytest.raises(ValueError, match="exclusion list of user 1"):
        rt.rank_metrics_matrixfree_check(ok, _mask([[], [6, 6], []], 10))


def test_an_id_outside_the_table_is_an_index_error():
    ok = _mask([[1, 2], []], 10)
    with pytest.raises(IndexError, match="user 1"):
        rt.rank_metrics_matrixfree_check(ok, _mask([[0], [3, 10]], 10))
    with pytest.raises(IndexError):
        rt.rank_metrics_matrixfree_check(_mask([[-1, 2], []], 10), ok)


def test_bad_query_arguments():
    with pytest.raises(ValueError):
        rt.rank_metrics_matrixfree_scratch(10, 0, 64, "dot", 1, 1)
    with pytest.raises(ValueError):
        rt.rank_metrics_matrixfree_scratch(10, 100, 64, "dot", 101, 1)


@pytest.mark.parametrize("kind", ["dot", "gmf"])
@pytest.mark.parametrize("n,items", [(1000, 10 ** 6), (100000, 50 * 10 ** 6)])
def test_the_scratch_stays_within_the_budget(n, items, kind):
    for budget, limit in ((0, 512 * MB), (64 * MB, 64 * MB), (4 * MB, 4 * MB)):
        nbytes, per = rt.rank_metrics_matrixfree_scratch(n, items, 64, kind, 20, 200, budget)
        assert 0 < nbytes <= limit and per >= 1


def test_l2_rows_are_bounded_by_the_budget_too():
    nbytes, per = rt.rank_metrics_matrixfree_scratch(1000, 10 ** 6, 64, "l2", 20, 200)
    assert nbytes <= 512 * MB and per >= 1 and nbytes < 1000 * 10 ** 6 * 4 // 4
    # not even the smallest batch fits: the query says what that batch takes (65 score rows: the scorer's wide tile)
    nbytes, per = rt.rank_metrics_matrixfree_scratch(100000, 50 * 10 ** 6, 64, "l2", 20, 200)
    assert per == 1 and nbytes > 512 * MB and nbytes < 70 * 50 * 10 ** 6 * 4


@pytest.mark.parametrize("kind", ["dot", "gmf"])
def test_ten_times_the_items_does_not_break_the_budget(kind):
    n = 1000
    for items in (10 ** 5, 10 ** 6):
        a, per_a = rt.rank_metrics_matrixfree_scratch(n, items, 64, kind, 20, 200)
        b, per_b = rt.rank_metrics_matrixfree_scratch(n, 10 * items, 64, kind, 20, 200)
        assert a <= 512 * MB and b <= 512 * MB and per_a >= 1 and per_b >= 1
        assert a == b and per_a == per_b == n               # nothing in it grows with the item count
