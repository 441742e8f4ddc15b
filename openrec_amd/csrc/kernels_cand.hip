// Scores and ranking metrics of each user's CANDIDATE LIST (orx_score_candidates, orx_rank_metrics_candidates): the work
// grows with the listed items, never with users x items.
//
// Semantics.  A score equals, bit for bit, the element orx_score_all_items writes for that (user, item).  The metrics of a user
// equal, bit for bit, what orx_rank_metrics_csr returns for the same positives and the exclusion list [0, items) \ cand
// (kernels_eval.hip states them): AUC over cand \ pos on the raw scores, the rank counts on expf of the scores with the exact
// test where expf rounds neighbours together, a positive outside cand ranked against every candidate with expf > 0,
// 0 / 0 -> NaN, the per-user sums added in rank_finish_kernel's order.
//
// cand_score_kernel (dot / GMF, dim <= 128) is a random gather of item rows: 4 D bytes per entry, plus 4 for the id, 4 for the
// bias and 4 written.  The lists of a batch are one flat run of entries cut into tiles of 16, whoever owns them, so a user
// with 20 candidates does not own a workgroup.  A tile is one 16 x 16 MFMA tile: row i holds the item of entry i, column j the
// user row of entry j (times w for GMF), and entry i's score is the DIAGONAL element [i][i].  The products go through
// __builtin_amdgcn_mfma_f32_16x16x4f32 with the scorer's operand layout and k order; an MFMA output element's bits do not
// depend on its place in the tile or on the other rows and columns (kernels_evalmf.hip), so these are the scorer's bits.
//   loads     lane (i, kq) reads columns 16 kb + 4 kq .. + 3 of item row i as one 16-byte load (dim % 4 == 0; scalar loads
//             otherwise): the four lanes of a row read 64 contiguous bytes per k block
//   user row  each lane keeps its column's user fragment in registers and reloads it only when its entry's user changes: a
//             wavefront inside one long list fetches the user row once, not once per tile
//   in flight a wavefront owns a run of consecutive tiles; the next tile's item rows and bias and the id of the tile after it
//             are loaded before the current tile's MFMAs; 5 wavefronts per SIMD at dim 64, 3 at dim 128
// cand_rank_kernel, one workgroup per user: the chunk's thresholds sorted as rank_thresholds sorts them, the candidates'
// scores staged in LDS in pieces of CAND_CAP with their "is a positive" flag (a search in the ascending positive list), bucket
// counts and corrections in LDS integers, then one thread adds the float sums in rank_finish_kernel's order.  No global atomics.
//
// L2 scores, dim > 128 and ORX_SCORE_SIMPLE take a bounded dense route (api_cand.hip): the scorer itself writes the score
// rows of a batch of users and cand_pick_kernel picks the listed entries out of them -- L2 norm sums are only bit-stable within
// the scorer's own kernel body (kernels_topk.hip).  That route does not save compute; it still removes the dense masks.
#include <algorithm>

#include "orx_device.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CAND_CAP = 2048;      // candidate scores of one user staged in LDS at a time

__device__ __forceinline__ bool cand_in_sorted(const int32_t* e, int64_t ne, int32_t id) {
    int64_t lo = 0, hi = ne;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (e[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo < ne && e[lo] == id;
}

// the user whose list holds flat entry e: the first q with ptr[q + 1] > e (empty lists are stepped over); e < ptr[nq]
__device__ __forceinline__ int64_t cand_owner(const int64_t* ptr, int64_t nq, int64_t e) {
    int64_t lo = 0, hi = nq - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ptr[mid + 1] <= e) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------ scorer ---
template <int KB, bool VEC>
__device__ __forceinline__ void cand_load_row(const float* base, int D, int kq, bool have, f32x4 (&r)[KB]) {
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
        const int col = 16 * kb + 4 * kq;
        f32x4 z = {0.f, 0.f, 0.f, 0.f};
        if (VEC) {
            if (have && col < D) z = *reinterpret_cast<const f32x4*>(base + col);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) if (have && col + c < D) z[c] = base[col + c];
        }
        r[kb] = z;
    }
}

template <int KB, bool VEC>
__global__ __launch_bounds__(256) void cand_score_kernel(CandScoreArgs a, int gmf, int64_t tiles_per_wave) {
    const int lane = threadIdx.x & 63, ii = lane & 15, kq = lane >> 4;
    const int64_t ntiles = (a.E + 15) >> 4;
    const int64_t t0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * tiles_per_wave;
    const int64_t t1 = t0 + tiles_per_wave < ntiles ? t0 + tiles_per_wave : ntiles;
    if (t0 >= t1) return;
    const int D = a.D;
    const bool diag = kq == (ii >> 2);                     // this lane holds element [ii][ii] of the tile in acc[ii & 3]
    auto load_id = [&](int64_t t) -> int { const int64_t e = t * 16 + ii; return (t < t1 && e < a.E) ? a.items[e] : -1; };
    f32x4 cur[KB], nxt[KB], uf[KB];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) uf[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
    int item = load_id(t0);
    cand_load_row<KB, VEC>(a.V + (size_t)(item < 0 ? 0 : item) * D, D, kq, item >= 0, cur);
    float bcur = (a.b && diag && item >= 0) ? a.b[item] : 0.f;
    int item_n = load_id(t0 + 1);
    int64_t q = -1, qend = 0;                              // the user of this lane's entry: ptr[q] <= e < qend = ptr[q + 1]
    for (int64_t t = t0; t < t1; ++t) {
        cand_load_row<KB, VEC>(a.V + (size_t)(item_n < 0 ? 0 : item_n) * D, D, kq, item_n >= 0, nxt);
        const float bnxt = (a.b && diag && item_n >= 0) ? a.b[item_n] : 0.f;
        const int item_nn = load_id(t + 2);
        const int64_t e = t * 16 + ii;
        if (item >= 0 && e >= qend) {                      // (a lane beyond the last entry keeps whatever fragment it has)
            if (q < 0) q = cand_owner(a.ptr, a.nq, e);
            else do ++q; while (a.ptr[q + 1] <= e);
            qend = a.ptr[q + 1];
            const float* urow = a.U + (size_t)a.uid[q] * D;
            cand_load_row<KB, VEC>(urow, D, kq, true, uf);
            if (gmf) {
                f32x4 wf[KB];
                cand_load_row<KB, VEC>(a.w, D, kq, true, wf);
#pragma unroll
                for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                    for (int c = 0; c < 4; ++c) uf[kb][c] *= wf[kb][c];
            }
        }
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[kb][c], uf[kb][c], acc, 0, 0, 0);
        // acc[r] = item of entry 4 (lane / 16) + r against the user of entry lane % 16
        if (diag && item >= 0) {
            const int r = ii & 3;
            const float x = r == 0 ? acc[0] : (r == 1 ? acc[1] : (r == 2 ? acc[2] : acc[3]));
            a.out[e] = a.b ? x + bcur : x;
        }
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) cur[kb] = nxt[kb];
        bcur = bnxt; item = item_n; item_n = item_nn;
    }
}

// the dense route: entry e of user q out of the score rows the scorer wrote for the batch
__global__ __launch_bounds__(256) void cand_pick_kernel(const float* rows, int64_t NI, const int64_t* ptr, const int32_t* items,
                                                        int64_t nq, int64_t E, float* out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int64_t q = cand_owner(ptr, nq, e);
    out[e] = rows[(size_t)q * NI + items[e]];
}

// ------------------------------------------------------------------------------------------ ranker ---
// rank_sweep_kernel's helpers restated (as kernels_evalmf.hip restates them)
__device__ __forceinline__ int cand_bucket(const float* T, int NB, float sj) {
    int d = 0;
    for (int h = NB >> 1; h >= 1; h >>= 1) d += (T[d + h] < sj) ? h : 0;
    return d;
}

__global__ __launch_bounds__(256) void cand_rank_kernel(CandRankArgs a) {
    __shared__ float T[64], raw_s[64];
    __shared__ int tex[64], raw_ex[64];
    __shared__ unsigned hist[64], corr[64], gtp[64];
    __shared__ unsigned nz_s, inter_s;
    __shared__ float cs[CAND_CAP];
    __shared__ unsigned char cp[CAND_CAP];
    const int NB = a.NB, NT = NB - 1;
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t p0 = a.pos_ptr[q], c0 = a.cand_ptr[q];
    const int n_pos = (int)(a.pos_ptr[q + 1] - p0);
    const int64_t nc = a.cand_ptr[q + 1] - c0;
    const int32_t* pi = a.pos_items + p0;
    const int32_t* ci = a.cand_items + c0;
    const bool one_piece = nc <= CAND_CAP;
    if (tid == 0) inter_s = 0u;
    __syncthreads();
    {                                                               // candidates that are positives: n_eval = |cand \ pos|
        unsigned both = 0;
        for (int64_t m = tid; m < n_pos; m += 256) both += cand_in_sorted(ci, nc, pi[m]) ? 1u : 0u;
        for (int off = 32; off > 0; off >>= 1) both += __shfl_xor(both, off);
        if (lane == 0 && both) atomicAdd(&inter_s, both);
    }
    float auc_sum = 0.0f, nd[16], rc[16];                           // thread 0's
    for (int t = 0; t < 16; ++t) { nd[t] = 0.0f; rc[t] = 0.0f; }
    for (int k0 = 0; k0 < n_pos; k0 += NT) {                        // a chunk of NT positives, as the call's sweeps take them
        const int pc = min(NT, n_pos - k0);
        __syncthreads();
        if (tid < 64) { hist[tid] = 0u; corr[tid] = 0u; gtp[tid] = 0u; }
        if (tid < NT) {
            const bool have = tid < pc;
            raw_s[tid] = have ? a.pos_s[p0 + k0 + tid] : INFINITY;
            raw_ex[tid] = have && !cand_in_sorted(ci, nc, pi[k0 + tid]);        // a positive outside cand is an excluded positive
        }
        if (tid == 0) { T[0] = -INFINITY; nz_s = 0u; }
        __syncthreads();
        if (tid < NT) {                                             // rank_thresholds: sorted by (score, list index)
            const float x = raw_s[tid];
            int r = 0;
            for (int m = 0; m < NT; ++m) r += (raw_s[m] < x) || (raw_s[m] == x && m < tid);
            T[1 + r] = x; tex[r] = raw_ex[tid];
        }
        __syncthreads();
        unsigned nz = 0;
        for (int64_t b0 = 0; b0 < nc; b0 += CAND_CAP) {
            const int len = (int)min((int64_t)CAND_CAP, nc - b0);
            if (!(one_piece && k0 > 0)) {
                __syncthreads();
                for (int i = tid; i < len; i += 256) {
                    cs[i] = a.cand_s[c0 + b0 + i];
                    cp[i] = cand_in_sorted(pi, n_pos, ci[b0 + i]) ? 1 : 0;
                }
                __syncthreads();
            }
            for (int i = tid; i < len; i += 256) {
                const float sj = cs[i];
                nz += (sj < -80.0f && !(expf(sj) > 0.0f)) ? 0u : 1u;          // exp(pred) > 0: what an excluded positive is ranked against
                if (cp[i]) continue;
                const int d = cand_bucket(T, NB, sj);
                atomicAdd(&hist[d], 1u);
                if (sj - T[d] < 1e-6f || sj > 88.0f || sj < -80.0f) {          // rank_sweep_kernel's exact test
                    const float vj = expf(sj);
                    int c = d;
                    while (c > 0 && (sj - T[c] < 1e-6f || sj > 88.0f || sj < -87.0f)) {
                        if (expf(T[c]) >= vj) --c; else break;
                    }
                    for (int m = c; m < d; ++m) atomicAdd(&corr[m], 1u);
                }
            }
        }
        // the positives themselves are ranked against too (they are not excluded from rank_above)
        for (int m = tid; m < n_pos; m += 256) {
            if (!cand_in_sorted(ci, nc, pi[m])) continue;
            const float vm = expf(a.pos_s[p0 + m]);
            for (int k = 0; k < pc; ++k) if (vm > expf(T[1 + k])) atomicAdd(&gtp[k], 1u);
        }
        for (int off = 32; off > 0; off >>= 1) nz += __shfl_xor(nz, off);
        if (lane == 0 && nz) atomicAdd(&nz_s, nz);
        __syncthreads();
        if (tid == 0) {                                             // one thread, rank_finish_kernel's order of the float sums
            unsigned below = 0, all = 0;
            for (int d = 0; d < NB; ++d) all += hist[d];
            for (int k = 0; k < pc; ++k) {
                below += hist[k];
                const unsigned above = tex[k] ? nz_s : (all - below) - corr[k] + gtp[k];
                auc_sum += (float)below;
                const float g = (float)above;
                const float lr = 1.0f / (logf(g + 2.0f) / logf(2.0f));
                for (int t = 0; t < a.nat; ++t)
                    if (g < a.at[t]) { nd[t] += lr; rc[t] += 1.0f; }
            }
        }
    }
    if (tid == 0) {
        const int neval = (int)(nc - (int64_t)inter_s);
        a.auc[q] = auc_sum / ((float)n_pos * (float)neval);         // (0 / 0 -> NaN like TF)
        for (int t = 0; t < a.nat; ++t) {
            a.ndcg[q * a.nat + t] = nd[t];
            a.recall[q * a.nat + t] = rc[t] / (float)n_pos;
        }
    }
}

// ------------------------------------------------------------------------------------------ launchers ---
bool orx_cand_has_tile(int D) { return D >= 1 && D <= 128; }

int orx_launch_cand_score(orx_ctx* ctx, const CandScoreArgs& a, int kind) {
    if (a.E == 0 || a.nq == 0) return ORX_OK;
    ORX_ARG(kind == 0 || kind == 2, "candidate scorer: L2 scores take the dense route");
    ORX_ARG(orx_cand_has_tile(a.D), "candidate scorer: no tile for dim %d", a.D);
    int KB = 1;
    while (16 * KB < a.D) KB *= 2;
    const bool vec = (a.D & 3) == 0;
    const int64_t ntiles = (a.E + 15) / 16;
    // a run of tiles per wavefront: long enough to keep a user row, short enough for about 16 K wavefronts
    const int64_t tpw = std::max<int64_t>(8, (ntiles + 16383) / 16384);
    const int64_t waves = (ntiles + tpw - 1) / tpw;
    const dim3 g((unsigned)((waves + 3) / 4));
    const int gmf = kind == 2 ? 1 : 0;
    ProfScope ps(ctx, ORX_K_GEMM);
#define ORX_CS(B) do { if (vec) ORX_LAUNCH(ctx, (cand_score_kernel<B, true>), g, dim3(256), 0, a, gmf, tpw); \
                       else ORX_LAUNCH(ctx, (cand_score_kernel<B, false>), g, dim3(256), 0, a, gmf, tpw); } while (0)
    switch (KB) { case 1: ORX_CS(1); break; case 2: ORX_CS(2); break; case 4: ORX_CS(4); break; default: ORX_CS(8); break; }
#undef ORX_CS
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

int orx_launch_cand_pick(orx_ctx* ctx, const float* rows, int64_t NI, const int64_t* ptr, const int32_t* items, int64_t nq,
                         int64_t E, float* out) {
    if (E == 0 || nq == 0) return ORX_OK;
    ORX_LAUNCH(ctx, cand_pick_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, rows, NI, ptr, items, nq, E, out);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

int orx_launch_cand_rank(orx_ctx* ctx, const CandRankArgs& a, int64_t nq) {
    if (nq == 0) return ORX_OK;
    ORX_LAUNCH(ctx, cand_rank_kernel, dim3((unsigned)nq), dim3(256), 0, a);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}
