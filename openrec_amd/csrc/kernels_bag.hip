// Pooling of per-call ragged item lists -- an EmbeddingBag in its (input, offsets) form -- and the two small kernels that carry its
// backward through the sorted apply (orx_bag_pool / orx_seqrec_step / orx_seqrec_loss, include/openrec_hip.h has the semantics).
//
//   q_i = c_i * sum over e in [ptr[i], ptr[i + 1]), in list order, of H[items[e]]          c_i = 1 / len_i  |  1 / denom
//
// bag_pool_kernel.  One wavefront per bag, whatever its length.  The wavefront fetches 64 ids of its bag with one coalesced load
// and hands them to its lanes by shuffles, so a row address never waits for a per-lane id load.  A row of D = 4 k floats is
// LPR = max(D / 4, 4) lanes (rounded up to a power of two) x float4, so a load instruction holds G = 64 / LPR rows (D = 64: four
// rows of 256 B) and BAG_UN such instructions are in flight before the adds.  Lane group g adds the entries g, g + G, g + 2 G, ...
// of the bag in that order into its own float4; the G group sums are combined by a butterfly over the lane groups (xor 32, 16,
// ... LPR), the same tree in every lane.  Other dims (D % 4 != 0, or rows that do not start on 16 bytes): one row per load, lane l
// holds columns l, l + 64, l + 128 and l + 192, the entries are added in list order.  Either way the order of the additions is a
// function of (len_i, D) alone: the bits of q_i do not depend on B, on the other bags or on where the output row lies.  c_i is
// rounded once, the product once.  No atomics.
//
// This is the walk of graph_row_kernel (kernels_graph.hip) without what a CSR product needs and a bag does not -- column scales
// (a multiply per entry), 64-bit offsets, segments of long rows summed by other wavefronts -- and with what a bag needs and the
// product does not: dims up to 256, ids handed out by shuffles, the owner of every list position for the backward, and a bag
// that DIES as a whole on a bad id (the product drops the entry).  DESIGN.md "History-pooled sequence recommender" has the numbers.
//
// A bag whose offsets are malformed (negative, decreasing, beyond n, ptr[0] != 0, ptr[B] != n) or that holds an id outside H is
// never used as an address: its q_i is +0, its coefficient 0, its sample id -1 -- the gradient launch then drops the sample by its
// own rule -- and the context's index flag is raised.
#include "orx_device.h"

namespace {

constexpr int BAG_UN = 4;          // row-load instructions in flight per wavefront

// what both walks share: the bag's bounds, checked
struct BagSpan { int64_t lo; int64_t len; bool bad; };

__device__ __forceinline__ BagSpan bag_span(const BagArgs& a, int64_t i) {
    const int64_t lo = a.ptr[i], hi = a.ptr[i + 1];
    BagSpan s;
    s.bad = lo < 0 || hi < lo || hi > a.n || (i == 0 && lo != 0) || (i == a.B - 1 && hi != a.n);
    s.lo = lo; s.len = s.bad ? 0 : hi - lo;
    return s;
}

// ids [c0, c0 + 64) of the bag, one per lane: -1 where the bag ends or the id lies outside H (*bad then); the owner of the position
__device__ __forceinline__ int bag_ids(const BagArgs& a, const BagSpan& sp, int64_t i, int64_t c0, int lane, bool* bad) {
    int id = -1;
    if (c0 + lane < sp.len) {
        const int64_t e = sp.lo + c0 + lane;
        id = a.items[e];
        if (!id_ok(id, a.rows)) { id = -1; *bad = true; }
        if (a.owner) a.owner[e] = (int32_t)i;
    }
    return id;
}

// c_i and what the step keeps of the bag; -> the scale of the sum (0: an empty or a dead bag)
__device__ __forceinline__ float bag_finish(const BagArgs& a, const BagSpan& sp, int64_t i, bool bad, int lane) {
    const bool dead = __ballot(bad) != 0ull;
    float c = 0.0f;
    if (!dead && sp.len > 0) c = a.mode == ORX_BAG_MEAN ? 1.0f / (float)sp.len : a.inv_denom;
    if (lane == 0) {
        if (dead) *a.err = 1;
        if (a.uid) a.uid[i] = dead ? -1 : (int32_t)i;
        if (a.coef) a.coef[i] = c;
    }
    return c;
}

template <int LPR>
__global__ __launch_bounds__(256) void bag_pool_kernel(BagArgs a) {
    constexpr int G = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.B) return;
    const int sub = lane % LPR, grp = lane / LPR, col = 4 * sub;
    const bool act = col < a.D;
    const BagSpan sp = bag_span(a, i);
    bool bad = sp.bad;
    f4 s = {0.f, 0.f, 0.f, 0.f};
    for (int64_t c0 = 0; c0 < sp.len; c0 += 64) {
        const int cnt = (int)(sp.len - c0 < 64 ? sp.len - c0 : 64);
        const int mine = bag_ids(a, sp, i, c0, lane, &bad);
        for (int j0 = 0; j0 * G < cnt; j0 += BAG_UN) {                  // (64 / G is a multiple of BAG_UN: k stays below 64)
            f4 x[BAG_UN];
#pragma unroll
            for (int u = 0; u < BAG_UN; ++u) {
                const int k = (j0 + u) * G + grp;
                const int id = __shfl(mine, k);
                x[u] = f4{0.f, 0.f, 0.f, 0.f};
                if (k < cnt && id >= 0 && act) x[u] = *reinterpret_cast<const f4*>(a.H + (size_t)id * a.D + col);
            }
#pragma unroll
            for (int u = 0; u < BAG_UN; ++u)
                if ((j0 + u) * G + grp < cnt) { s.x += x[u].x; s.y += x[u].y; s.z += x[u].z; s.w += x[u].w; }
        }
    }
#pragma unroll
    for (int off = 32; off >= LPR; off >>= 1) {
        s.x += __shfl_xor(s.x, off); s.y += __shfl_xor(s.y, off); s.z += __shfl_xor(s.z, off); s.w += __shfl_xor(s.w, off);
    }
    const float c = bag_finish(a, sp, i, bad, lane);
    if (grp == 0 && act) {
        f4 q = {0.f, 0.f, 0.f, 0.f};
        if (c != 0.0f) q = f4{c * s.x, c * s.y, c * s.z, c * s.w};
        *reinterpret_cast<f4*>(a.out + (size_t)i * a.D + col) = q;
    }
}

// any D <= 256: lane l holds columns l + 64 e, the entries are added in list order
__global__ __launch_bounds__(256) void bag_pool_generic_kernel(BagArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.B) return;
    const BagSpan sp = bag_span(a, i);
    bool bad = sp.bad;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t c0 = 0; c0 < sp.len; c0 += 64) {
        const int cnt = (int)(sp.len - c0 < 64 ? sp.len - c0 : 64);
        const int mine = bag_ids(a, sp, i, c0, lane, &bad);
        for (int j0 = 0; j0 < cnt; j0 += BAG_UN) {
            float x[BAG_UN][4];
#pragma unroll
            for (int u = 0; u < BAG_UN; ++u) {
                const int id = __shfl(mine, (j0 + u) & 63);
                const bool live = j0 + u < cnt && id >= 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) x[u][e] = (live && lane + 64 * e < a.D) ? a.H[(size_t)id * a.D + lane + 64 * e] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < BAG_UN; ++u)
                if (j0 + u < cnt) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[e] += x[u][e];
                }
        }
    }
    const float c = bag_finish(a, sp, i, bad, lane);
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (lane + 64 * e < a.D) a.out[(size_t)i * a.D + lane + 64 * e] = c != 0.0f ? c * s[e] : 0.0f;
}

// g[i][0 .. D) *= coef[i]: the gradient row every occurrence of bag i takes, each element rounded once
__global__ __launch_bounds__(256) void bag_scale_rows_kernel(float* __restrict__ g, const float* __restrict__ coef, int64_t B, int D, int gs) {
    const int64_t total = B * D, stride = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
        const int64_t i = t / D;
        const size_t at = (size_t)i * gs + (size_t)(t - i * D);
        g[at] = coef[i] * g[at];
    }
}

// the sorted (row, list position) pairs with the position replaced by the bag that owns it: owners never decrease along the
// list, so a row's occurrences keep their list order.  A position no well-formed bag covers (a malformed device list: the call
// fails with the index error) takes bag 0 -- an address inside the gradient rows.
__global__ __launch_bounds__(256) void bag_owner_pairs_kernel(const uint2* __restrict__ sorted, const int32_t* __restrict__ owner, int64_t n,
                                                              int64_t B, uint2* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += stride) {
        const uint2 e = sorted[k];
        uint32_t o = e.y < (uint64_t)n ? (uint32_t)owner[e.y] : 0u;
        if (o >= (uint64_t)B) o = 0u;
        out[k] = make_uint2(e.x, o);
    }
}

inline int bag_lpr(const BagArgs& a) {       // 0: the plain walk
    if (a.D % 4 != 0 || a.D > 256 || (uintptr_t)a.H % 16 != 0 || (uintptr_t)a.out % 16 != 0) return 0;
    int lpr = 4;
    while (4 * lpr < a.D) lpr *= 2;
    return lpr;
}

inline unsigned bag_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 256 * 32)); }

}  // namespace

int orx_launch_bag_pool(orx_ctx* ctx, const BagArgs& a) {
    if (a.B == 0) return ORX_OK;
    ProfScope ps(ctx, ORX_K_FUSED);
    const dim3 g((unsigned)((a.B + 3) / 4));
    switch (bag_lpr(a)) {
        case 4: ORX_LAUNCH(ctx, bag_pool_kernel<4>, g, dim3(256), 0, a); break;
        case 8: ORX_LAUNCH(ctx, bag_pool_kernel<8>, g, dim3(256), 0, a); break;
        case 16: ORX_LAUNCH(ctx, bag_pool_kernel<16>, g, dim3(256), 0, a); break;
        case 32: ORX_LAUNCH(ctx, bag_pool_kernel<32>, g, dim3(256), 0, a); break;
        case 64: ORX_LAUNCH(ctx, bag_pool_kernel<64>, g, dim3(256), 0, a); break;
        default: ORX_LAUNCH(ctx, bag_pool_generic_kernel, g, dim3(256), 0, a); break;
    }
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

int orx_launch_bag_scale_rows(orx_ctx* ctx, float* g, const float* coef, int64_t B, int D, int gs) {
    if (B == 0) return ORX_OK;
    ProfScope ps(ctx, ORX_K_DUPAPPLY);
    ORX_LAUNCH(ctx, bag_scale_rows_kernel, dim3(bag_grid(B * D)), dim3(256), 0, g, coef, B, D, gs);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

int orx_launch_bag_owner_pairs(orx_ctx* ctx, const uint2* sorted, const int32_t* owner, int64_t n, int64_t B, uint2* out) {
    if (n == 0) return ORX_OK;
    ProfScope ps(ctx, ORX_K_DEDUP);
    ORX_LAUNCH(ctx, bag_owner_pairs_kernel, dim3(bag_grid(n)), dim3(256), 0, sorted, owner, n, B, out);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}
