"""Top-K recommendation, the parts that need no device: the new entry points are declared, exported and typed, the
TensorFlow shim exposes tf.math.top_k / tf.nn.top_k, and the argument checks made before any device call raise the
documented errors."""
import numpy as np
import pytest

from openrec_amd import _ffi
from openrec_amd import runtime as rt
from openrec_amd.tf2 import compat


def test_the_entry_points_are_exported_and_typed():
    lib = _ffi.load()
    for name in ("orx_recommend_topk", "orx_topk_rows"):
        assert hasattr(lib, name)
        assert name in _ffi.SIGNATURES
    assert len(_ffi.SIGNATURES["orx_recommend_topk"][1]) == 14
    assert len(_ffi.SIGNATURES["orx_topk_rows"][1]) == 10
    assert _ffi.ORX_OUT_DEVICE == 32


def test_the_shim_has_top_k():
    assert compat.tf.math.top_k is compat.top_k and compat.tf.nn.top_k is compat.top_k
    res = compat.TopKV2(values=1, indices=2)
    assert res.values == 1 and res.indices == 2


@pytest.mark.parametrize("k", [0, -1, 1025])
def test_k_outside_the_range_is_a_value_error(k):
    with pytest.raises(ValueError, match="k"):
        rt.topk_rows(np.zeros((2, 3), np.float32), k)


def test_top_k_rank_and_k_checks():
    with pytest.raises(NotImplementedError, match="rank 3"):
        compat.top_k(np.zeros((2, 3, 4), np.float32), 1)
    with pytest.raises(NotImplementedError, match="rank 0"):
        compat.top_k(np.float32(1.0), 1)
    with pytest.raises(ValueError, match="k = 5"):
        compat.top_k(np.zeros((2, 4), np.float32), 5)
    with pytest.raises(ValueError, match="k = 4"):
        compat.top_k(np.zeros(3, np.float32), 4)
    with pytest.raises(ValueError):
        compat.top_k(np.zeros(3, np.float32), -1)


def test_top_k_of_zero_is_empty():
    v, i = compat.top_k(np.zeros((2, 4), np.float32), 0)
    assert v.shape == (2, 0) and i.shape == (2, 0) and v.dtype == np.float32 and i.dtype == np.int32


def test_topk_rows_wants_two_dims():
    with pytest.raises(ValueError, match="shape"):
        rt.topk_rows(np.zeros(4, np.float32), 1)
