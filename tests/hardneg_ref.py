"""NumPy uint64 restatement of the sampler's stream (orx_sampler_device.h) and of the hard-negative selection rule
(kernels_hardneg.hip), shared by tests/test_hardneg_cpu.py, tests/test_gpu_hardneg.py and the other sampler tests.

Sample g of stream `seed`: the record perm_e(g mod R) of epoch e = g // R (keyed 4-round Feistel permutation with cycle walking)
gives (u, p); candidate c is a uniform item re-drawn (at most 256 attempts) while it is a positive of u, keyed by
    seed_c = seed if c == 0 else mix64(seed + c * 0xD1B54A32D192ED03)
    cand   = mix64(seed_c ^ (g * 0x9E3779B97F4A7C15) ^ (attempt << 56) ^ 0xA5A5A5A5) % total_items
so candidate 0 is the negative of the plain pairwise sampler."""
import numpy as np

U64 = np.uint64
MASK64 = (1 << 64) - 1


def mix64(x):
    x = np.asarray(x, U64)
    with np.errstate(over="ignore"):
        x = x + U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
        return x ^ (x >> U64(31))


def feistel_perm(x, n, h, key):
    """keyed permutation of [0, n) applied to the array x (entries < n); key: array like x or a scalar"""
    x = np.array(x, U64)
    key = np.broadcast_to(np.asarray(key, U64), x.shape)
    mask = U64((1 << h) - 1)
    todo = np.ones(x.shape, bool)
    while todo.any():
        xs, ks = x[todo], key[todo]
        l, r = xs >> U64(h), xs & mask
        for rnd in range(4):
            with np.errstate(over="ignore"):
                f = mix64(r ^ (ks + U64((0x632BE59BD9B4E019 * (rnd + 1)) & MASK64))) & mask
            l, r = r, l ^ f
        x[todo] = (l << U64(h)) | r
        todo = x >= U64(n)
    return x


def make_data(seed=0, NU=500, NI=300, NR=7001):
    """the records of test_sampler_contract: user 3 has 60 positives (20 % of the items)"""
    rng = np.random.default_rng(seed)
    raw = np.zeros(NR, dtype=[("user_id", np.int32), ("item_id", np.int32)])
    raw["user_id"] = rng.integers(0, NU, NR); raw["item_id"] = rng.integers(0, NI, NR)
    raw[:60]["user_id"] = 3; raw[:60]["item_id"] = np.arange(60)
    return raw


def positive_keys(raw, NI):
    return np.unique(raw["user_id"].astype(np.int64) * NI + raw["item_id"])


def records(raw, seed, g):
    """(u, p) of the samples g (int array)"""
    R = len(raw)
    h = 1
    while (1 << (2 * h)) < R:
        h += 1
    g = np.asarray(g, U64)
    epoch, pos = g // U64(R), g % U64(R)
    with np.errstate(over="ignore"):
        key = mix64(U64(seed & MASK64) ^ (epoch * U64(0xD6E8FEB86659FD93)))
    rec = feistel_perm(pos, R, h, key).astype(np.int64)
    return raw["user_id"][rec].astype(np.int32), raw["item_id"][rec].astype(np.int32)


def candidates(raw, NI, seed, g, M, users=None):
    """-> (u, p, cand[len(g), M]) of the samples g"""
    g = np.asarray(g, np.int64)
    u, p = records(raw, seed, g)
    if users is not None:
        u = np.asarray(users, np.int32)
    keys = positive_keys(raw, NI)
    gu = g.astype(U64)
    out = np.zeros((len(g), M), np.int32)
    seed = U64(seed & MASK64)
    for c in range(M):
        with np.errstate(over="ignore"):
            seed_c = seed if c == 0 else mix64(seed + U64((c * 0xD1B54A32D192ED03) & MASK64))
            base = seed_c ^ (gu * U64(0x9E3779B97F4A7C15)) ^ U64(0xA5A5A5A5)
        todo = np.arange(len(g))
        for attempt in range(256):
            ng = (mix64(base[todo] ^ U64(attempt << 56)) % U64(NI)).astype(np.int64)
            out[todo, c] = ng
            k = u[todo].astype(np.int64) * NI + ng
            j = np.searchsorted(keys, k)
            hit = (j < len(keys)) & (keys[np.minimum(j, len(keys) - 1)] == k)
            todo = todo[hit]
            if len(todo) == 0:
                break
    return u, p, out


def select(scores):
    """the selection rule on fp32 scores [n, M] -> column: the largest score, the smallest column among equal ones; a NaN never
    wins against a number; all NaN: column 0"""
    s = np.asarray(scores, np.float32)
    nan = np.isnan(s)
    filled = np.where(nan, -np.inf, s)
    j = np.argmax(filled, axis=1)                       # first index of the maximum over the numbers (-inf counts as a number)
    # a row whose maximum over the numbers is -inf: the first true -inf if there is one, else (all NaN) column 0
    top = filled[np.arange(len(s)), j]
    low = np.isneginf(top)
    if low.any():
        real = ~nan[low]
        j[low] = np.where(real.any(axis=1), np.argmax(real, axis=1), 0)
    return j
