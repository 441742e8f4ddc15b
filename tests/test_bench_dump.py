"""bench.py --dump-outputs: the row sample and the files it writes (CPU only; the helpers need no device)."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("n_rows,width,budget", [(1_000_000, 64, 24 << 20), (1_000_000, 65, 24 << 20),
                                                 (33_800_000, 128, 32 << 20), (100, 64, 24 << 20), (1_000_000, 4096, 24 << 20)])
def test_the_row_sample_is_fixed_sorted_and_bounded(bench, n_rows, width, budget):
    ids = bench.dump_rows(n_rows, width, budget)
    assert ids.dtype == np.int32 and ids.ndim == 1
    assert np.array_equal(ids, bench.dump_rows(n_rows, width, budget))             # the same sample in every run
    assert len(ids) == min(n_rows, bench.DUMP_SAMPLE_ROWS, budget // (4 * width))
    assert np.all(np.diff(ids) > 0)                                                  # sorted, no row twice
    assert ids[0] >= 0 and ids[-1] < n_rows
    assert len(ids) * width * 4 <= budget


def test_outputs_are_written_as_float32_npy(bench, tmp_path):
    out = tmp_path / "dump"
    arrays = {"user_rows": np.arange(12, dtype=np.float64).reshape(3, 4), "item_bias": np.ones((3, 1), np.float32)}
    bench.dump_outputs(str(out), arrays)
    assert sorted(os.listdir(out)) == ["item_bias.npy", "user_rows.npy"]
    for k, v in arrays.items():
        got = np.load(out / (k + ".npy"))
        assert got.dtype == np.float32 and np.array_equal(got, v.astype(np.float32))


def test_more_than_64_mb_is_refused_before_anything_is_written(bench, tmp_path):
    out = tmp_path / "dump"
    too_big = {"a": np.zeros((32 << 20) // 4, np.float32), "b": np.zeros((32 << 20) // 4 + 1, np.float32)}
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(out), too_big)
    assert not out.exists() or os.listdir(out) == []
