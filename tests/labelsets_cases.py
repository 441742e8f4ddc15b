"""The seeded label sets of tests/test_labelsets_cpu.py and tests/test_gpu_labelsets.py, on the shapes of
tests/fullsoftmax_cases.py (B = 1, NI = 63 / 65, n_j > 1, ragged item and sample chunks, D = 50 and D = 256 are there already).

Sample i's set has LENS[i % 9] entries -- 0, 1, 2 .. 6, 65 and 130: the wavefront's 64-id load is crossed once and twice --, a
single sample has three.  Every non-empty set holds the item HOT of the case (the item-side run that every sample is in); every
set of two or more repeats its first entry (a duplicate is two entries); sets longer than the table repeat items by
themselves.  weights: per-entry weights uniform in (0.25, 2)."""
import numpy as np

import fullsoftmax_cases as fc

LENS = (0, 1, 2, 3, 4, 5, 6, 65, 130)
SHAPES, OPTS, LR, SCALE = fc.SHAPES, fc.OPTS, fc.LR, fc.SCALE
shape_case, make_bags, make_opt = fc.shape_case, fc.make_bags, fc.make_opt


def hot_item(case):
    return int(case["seed"] * 7 % case["NI"])


def set_lens(case):
    B = case["B"]
    return np.array([3] if B == 1 else [LENS[i % len(LENS)] for i in range(B)], np.int64)


def make_sets(case, weights=False, lens=None):
    """-> lptr int32 [B + 1], litems int32 [n_lab], lw float32 [n_lab] or None"""
    rng = np.random.default_rng(case["seed"] + 700)
    lens = set_lens(case) if lens is None else np.asarray(lens, np.int64)
    lptr = np.zeros(case["B"] + 1, np.int32)
    lptr[1:] = np.cumsum(lens)
    litems = rng.integers(0, case["NI"], int(lptr[-1])).astype(np.int32)
    hot = hot_item(case)
    for i, n in enumerate(lens):
        lo = lptr[i]
        if n >= 2:
            litems[lo + 1] = litems[lo]                 # a duplicate inside the set
        if n >= 1:
            litems[lo + n - 1] = hot                    # one item in every non-empty set
    lw = rng.uniform(0.25, 2.0, len(litems)).astype(np.float32) if weights else None
    return lptr, litems, lw


def make_seq(case):
    """-> H, V, b (b None without the bias table), bag ptr, bag items (bag 0 empty where B > 1)"""
    _, V, b, _, _ = fc.make(case)
    H = np.random.default_rng(case["seed"] + 900).uniform(-SCALE, SCALE, V.shape).astype(np.float32)
    ptr, items = fc.make_bags(case)
    return H, V, b, ptr, items


def padded(ptr, items, fill=-7, extra=2):
    """the ragged lists as the padded pair (seq [B, L], len [B]); the padding is never read"""
    lens = np.diff(ptr)
    seq = np.full((len(lens), int(lens.max(initial=0)) + extra), fill, np.int32)
    for i, n in enumerate(lens):
        seq[i, :n] = items[ptr[i]:ptr[i + 1]]
    return seq, lens.astype(np.int32)
