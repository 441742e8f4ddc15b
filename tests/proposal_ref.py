"""NumPy uint64 restatement of the sampler's draw from a weighted item proposal (smp_draw<true> of orx_sampler_device.h), shared by
tests/test_proposal_cpu.py and tests/test_gpu_proposal.py.  mix64, the (u, p) record stream and seed_c are tests/hardneg_ref.py's.

With an alias table (thr, alias), attempt a of candidate c of sample g is
    r    = mix64(seed_c ^ (g * 0x9E3779B97F4A7C15) ^ (a << 56) ^ 0xA5A5A5A5)      the word the uniform draw forms
    j    = r % total_items
    t    = uint32(mix64(r ^ 0x5851F42D4C957F2D) >> 32)
    item = j if t < thr[j] else alias[j]
re-drawn while item is a positive of the user; after 256 attempts the last draw is kept."""
import numpy as np

from hardneg_ref import MASK64, U64, mix64, positive_keys, records


def implied_probabilities(thr, alias):
    """q[i] of the table, exact, as integers in units of 1 / (n 2^32) (Python ints in an object array would be slow: the sums
    stay below n 2^32 <= 2^63 for n < 2^31, so int64 holds them)"""
    thr, alias = np.asarray(thr, np.uint32), np.asarray(alias, np.int64)
    n = len(thr)
    own = alias == np.arange(n)
    T = np.where(own, 1 << 32, thr.astype(np.int64))
    q = T.copy()
    other = ~own
    np.add.at(q, alias[other], (1 << 32) - T[other])
    return q


def candidates(raw, NI, seed, g, M, thr, alias, users=None):
    """-> (u, p, cand[len(g), M]) of the samples g under the proposal (thr, alias)"""
    thr, alias = np.asarray(thr, np.uint32), np.asarray(alias, np.int32)
    assert len(thr) == NI and len(alias) == NI
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
            r = mix64(base[todo] ^ U64(attempt << 56))
            j = (r % U64(NI)).astype(np.int64)
            t = (mix64(r ^ U64(0x5851F42D4C957F2D)) >> U64(32)).astype(np.uint32)
            ng = np.where(t < thr[j], j, alias[j].astype(np.int64))
            out[todo, c] = ng
            k = u[todo].astype(np.int64) * NI + ng
            at = np.searchsorted(keys, k)
            hit = (at < len(keys)) & (keys[np.minimum(at, len(keys) - 1)] == k)
            todo = todo[hit]
            if len(todo) == 0:
                break
    return u, p, out
