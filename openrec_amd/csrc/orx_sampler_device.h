// The device sampler's stream, stated once: every kernel that draws a record or a negative of (seed, g) calls these, so
// "candidate 0 of pairwise_hard is pairwise's negative", "pairwise_multi is the first N candidates of pairwise_hard" and
// "pairwise_weights is the weight of the record pairwise writes" hold by construction.  kernels_sampler.hip has the design;
// tests/hardneg_ref.py restates the stream in NumPy.
//   record    : sample g takes record perm_e(g mod R) of epoch e = g / R, perm_e a keyed 4-round Feistel permutation of [0, R)
//               with cycle walking, key mix64(seed ^ e * 0xD6E8FEB86659FD93)
//   candidate : seed_c  = c == 0 ? seed : mix64(seed + c * 0xD1B54A32D192ED03)
//               cand(c) = mix64(seed_c ^ (g * 0x9E3779B97F4A7C15) ^ (attempt << 56) ^ 0xA5A5A5A5) % total_items
//               re-drawn, at most 256 attempts, while it is a positive of the user (binary search in the sorted CSR row)
//   proposal  : PROP: the word r under the modulus picks the column j = r % total_items of the alias table and
//               t = (uint32)(mix64(r ^ 0x5851F42D4C957F2D) >> 32) takes j if t < thr[j], else alias[j]
// Only __device__ __forceinline__ functions: a kernel that calls them compiles to what it compiled to with the text in place.
#pragma once
#include "orx_device.h"

__device__ __forceinline__ uint64_t smp_mix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// keyed permutation of [0, n): 4-round Feistel on 2*h bits (2^(2h) >= n) + cycle walking
__device__ __forceinline__ uint64_t smp_feistel_perm(uint64_t x, uint64_t n, int h, uint64_t key) {
    const uint64_t mask = (1ull << h) - 1;
    do {
        uint64_t l = x >> h, r = x & mask;
#pragma unroll
        for (int round = 0; round < 4; ++round) {
            const uint64_t f = smp_mix64(r ^ (key + 0x632BE59BD9B4E019ull * (round + 1))) & mask;
            const uint64_t t = l ^ f;
            l = r; r = t;
        }
        x = (l << h) | r;
    } while (x >= n);
    return x;
}

// the record of position g of the stream (a sample, a head of the stratified stream, a per-pos group)
__device__ __forceinline__ uint64_t smp_rec(const SamplerArgs& a, uint64_t g) {
    const uint64_t epoch = g / (uint64_t)a.R, pos = g % (uint64_t)a.R;
    return smp_feistel_perm(pos, (uint64_t)a.R, a.h, smp_mix64(a.seed ^ (epoch * 0xD6E8FEB86659FD93ull)));
}

// candidate c of sample g, whose user is u
template <bool PROP>
__device__ __forceinline__ int smp_draw(const SamplerArgs& a, uint64_t g, int c, int u) {
    const uint64_t seed_c = c == 0 ? a.seed : smp_mix64(a.seed + (uint64_t)c * 0xD1B54A32D192ED03ull);
    const int64_t lo0 = a.ptr[u], hi0 = a.ptr[u + 1];
    int ng = 0;
    for (int attempt = 0; attempt < 256; ++attempt) {
        const uint64_t r = smp_mix64(seed_c ^ (g * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)attempt << 56) ^ 0xA5A5A5A5ull);
        ng = (int)(r % (uint64_t)a.total_items);
        if (PROP) {
            const uint2 rec = a.prop[ng];
            if (!((uint32_t)(smp_mix64(r ^ 0x5851F42D4C957F2Dull) >> 32) < rec.x)) ng = (int)rec.y;
        }
        int64_t lo = lo0, hi = hi0;                     // binary search: is ng a positive of u?
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (a.items[mid] < ng) lo = mid + 1; else hi = mid; }
        if (!(lo < hi0 && a.items[lo] == ng)) break;
    }
    return ng;
}

__device__ __forceinline__ bool smp_is_positive(const SamplerArgs& a, int u, int item) {
    const int64_t lo0 = a.ptr[u], hi0 = a.ptr[u + 1];
    int64_t lo = lo0, hi = hi0;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (a.items[mid] < item) lo = mid + 1; else hi = mid; }
    return lo < hi0 && a.items[lo] == item;
}
