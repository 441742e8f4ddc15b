"""NumPy uint64 / float32 restatement of the two pointwise producers' streams (kernels_sampler.hip: strat_emit_kernel,
perpos_kernel), on top of hardneg_ref's mix64, feistel_perm and records; shared by tests/test_pointwise_sampler_cpu.py and
tests/test_gpu_sampler.py.

stratified(seed, pos_ratio), from sample 0: sample g flips the coin
    float32(mix64(seed ^ g * 0xC2B2AE3D27D4EB4F ^ 0x1234567) >> 40) * 2^-24 <= float32(pos_ratio)
a head takes the record of position "heads before it" (hardneg_ref.records: the pairwise stream's keyed permutation, epoch by
epoch), label 1; a tail takes
    r = mix64(seed ^ g * 0x9E3779B97F4A7C15 ^ attempt << 56 ^ 0x5A5A5A5A),  u = (r >> 32) % users,  item = (r & 0xffffffff) % items
re-drawn (at most 256 attempts) while (u, item) is a positive pair, label 0.

per_pos_stratified(seed, pos_ratio), any g: groups of 1 + nneg samples, nneg = int((1 - pos_ratio) / pos_ratio) in doubles.
Group q = g // (nneg + 1) takes record q (label 1); its negatives are the first nneg values != p of
    feistel_perm(j, items, hi, mix64(seed ^ q * 0x9FB21C651E98DF25 ^ 0x77)),  j = 0 .. nneg,  hi the smallest with 4^hi >= items."""
import numpy as np

from hardneg_ref import MASK64, U64, feistel_perm, make_data, mix64, positive_keys, records

SPARSE = (500, 300, 701)            # users, items, records: users with empty rows
DENSE = (40, 30, 701)               # ~44 % of the 1200 cells are positive: the re-draw and the skip paths


def data(shape):
    """hardneg_ref.make_data's records for (users, items, records); its planted items are folded into the item range"""
    NU, NI, NR = shape
    raw = make_data(0, NU, NI, NR)
    raw["item_id"] %= NI
    return raw, NU, NI


def coins(seed, g, pos_ratio):
    """heads (bool) of the samples g"""
    g = np.asarray(g, U64)
    with np.errstate(over="ignore"):
        x = mix64(U64(seed & MASK64) ^ (g * U64(0xC2B2AE3D27D4EB4F)) ^ U64(0x1234567)) >> U64(40)
    return x.astype(np.float32) * np.float32(1.0 / 16777216.0) <= np.float32(pos_ratio)


def stratified(raw, NU, NI, seed, n, pos_ratio):
    """-> (uid, iid, label, attempts) of samples [0, n); attempts: draws a tail took (0 for a head)"""
    g = np.arange(n, dtype=np.int64)
    head = coins(seed, g, pos_ratio)
    uid, iid = np.zeros(n, np.int32), np.zeros(n, np.int32)
    attempts = np.zeros(n, np.int32)
    position = np.cumsum(head) - head                       # heads before it
    uid[head], iid[head] = records(raw, seed, position[head])
    keys = positive_keys(raw, NI)
    todo = np.flatnonzero(~head)
    with np.errstate(over="ignore"):
        base = U64(seed & MASK64) ^ (g.astype(U64) * U64(0x9E3779B97F4A7C15)) ^ U64(0x5A5A5A5A)
    for attempt in range(256):
        r = mix64(base[todo] ^ U64(attempt << 56))
        u = ((r >> U64(32)) % U64(NU)).astype(np.int64)
        it = ((r & U64(0xffffffff)) % U64(NI)).astype(np.int64)
        uid[todo], iid[todo] = u, it
        attempts[todo] = attempt + 1
        k = u * NI + it
        j = np.searchsorted(keys, k)
        hit = (j < len(keys)) & (keys[np.minimum(j, len(keys) - 1)] == k)
        todo = todo[hit]
        if len(todo) == 0:
            break
    return uid, iid, head.astype(np.float32), attempts


def per_pos_nneg(pos_ratio):
    return int((1.0 - float(pos_ratio)) / float(pos_ratio))


def per_pos(raw, NI, seed, g, pos_ratio):
    """-> (uid, iid, label, skipped) of the samples g (int array); skipped: the slot's group met a candidate equal to p at or
    before the slot's own candidate"""
    nneg = per_pos_nneg(pos_ratio)
    hi = 1
    while (1 << (2 * hi)) < NI:
        hi += 1
    g = np.asarray(g, np.int64)
    q, slot = g // (nneg + 1), g % (nneg + 1)
    u, p = records(raw, seed, q)
    with np.errstate(over="ignore"):
        key = mix64(U64(seed & MASK64) ^ (q.astype(U64) * U64(0x9FB21C651E98DF25)) ^ U64(0x77))
    item, taken = p.copy(), np.zeros(len(g), np.int64)
    skipped = np.zeros(len(g), bool)
    done = slot == 0
    for j in range(nneg + 1):
        c = feistel_perm(np.full(len(g), j, np.int64), NI, hi, key).astype(np.int32)
        same = c == p
        skipped |= same & ~done
        taken += ~same
        now = ~done & ~same & (taken == slot)
        item[now] = c[now]
        done |= now
    assert done.all()
    return u, item, (slot == 0).astype(np.float32), skipped
