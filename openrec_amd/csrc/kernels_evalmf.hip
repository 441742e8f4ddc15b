// Ranking metrics of the evaluation step without an [n, items] score matrix (orx_rank_metrics_matrixfree).
//
// Semantics: those of orx_rank_metrics_csr with the scorer (kernels_eval.hip states them): AUC on the raw scores, the rank
// counts on expf of the scores with the exact test where expf rounds neighbours together, an excluded positive ranked against
// every non-excluded item with expf > 0, 0 / 0 -> NaN.  The outputs equal the materialised path's bit for bit: both count
// the same integers from the same score bits and add them up in the same fixed order.
//
// Per batch of users and per chunk of NT = 2^STEPS - 1 positives (STEPS 3 / 4 / 6 from the call's longest positive list, as
// rank_sweep_kernel picks it):
//   0. gather     evalmf_gather_kernel, once per batch: the scores of every LISTED item (positives and exclusions) through the
//                 matrix cores with the scorer's operand layout and k order -- an MFMA output element's bits do not depend on
//                 its place in the tile, so these are the bits the sweep sees for the same (user, item).
//   1. thresholds evalmf_thresh_kernel: the chunk's positives sorted by (score, list index) into ts[user][NB], ts[0] = -inf.
//   2. sweep      evalmf_sweep_kernel: score_mfma_kernel restated statement for statement up to the epilogue (as
//                 topk_filter_kernel does); instead of the store every score finds its bucket d = #{thresholds < s} in the
//                 user's threshold table in LDS and bumps the user's bucket counter in LDS.  EVERY item is counted, masks
//                 ignored.  The rare item within 1e-6 of the threshold below it (or where expf overflows / leaves the normal
//                 range) takes rank_sweep_kernel's exact test and books corr[] / the expf == 0 count with global atomics.
//   3. finish     evalmf_finish_kernel, one wavefront per user: the listed items are taken out again -- each distinct item of
//                 P u E leaves the bucket (and the corr[] entries) its gathered score put it in, each excluded item leaves the
//                 expf > 0 count, |P u E| comes from searching each list in the other (both are strictly ascending) -- and
//                 the chunk's metric sums are added exactly as rank_finish_kernel adds them.
// No buffer grows with n x items: per user NB thresholds, 2 NB counters, the two lists and their scores.
// UCML (L2) scores, D > 128 and ORX_SCORE_SIMPLE take the scorer itself plus the existing sweeps in bounded user batches
// (api_evalmf.hip): L2 norm sums are only bit-stable within the scorer's own kernel body (kernels_topk.hip).  The L2 branches
// below are kept so that the sweep stays the scorer's statement for statement, but they are not instantiated.
#include "orx_device.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool evalmf_in_sorted(const int32_t* e, int64_t ne, int32_t id) {
    int64_t lo = 0, hi = ne;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (e[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo < ne && e[lo] == id;
}

// bucket of a score: d = #{thresholds < sj} (T[0] = -inf, unused thresholds +inf)
__device__ __forceinline__ int evalmf_bucket(const float* T, int NB, float sj) {
    int d = 0;
    for (int h = NB >> 1; h >= 1; h >>= 1) d += (T[d + h] < sj) ? h : 0;
    return d;
}

// does the item take the exact test of rank_sweep_kernel's slow path?
__device__ __forceinline__ bool evalmf_odd(float sj, float tb) { return sj - tb < 1e-6f || sj > 88.0f || sj < -80.0f; }

// the slow path of rank_sweep_kernel for one evaluated, non-excluded item in bucket d: c = the bucket expf puts it in
// (corr[m] counts it for c <= m < d); *drop: expf(sj) == 0, the item leaves the expf > 0 count
__device__ __forceinline__ int evalmf_exact(const float* T, float sj, int d, bool* drop) {
    const float vj = expf(sj);
    *drop = sj < -80.0f && !(vj > 0.0f);
    int c = d;
    while (c > 0 && (sj - T[c] < 1e-6f || sj > 88.0f || sj < -87.0f)) {
        if (expf(T[c]) >= vj) --c; else break;
    }
    return c;
}

// ------------------------------------------------------------------------------------------ listed items ---
// one wavefront per (user, list, 16 entries): a 16 x 16 MFMA tile whose 16 user columns all hold the user's row
__global__ __launch_bounds__(64) void evalmf_gather_kernel(EvalMfArgs a, int gmf) {
    const int64_t q = blockIdx.x;
    const int which = blockIdx.z;
    const int64_t* ptr = which ? a.excl_ptr : a.pos_ptr;
    const int32_t* items = which ? a.excl_items : a.pos_items;
    float* out = which ? a.excl_s : a.pos_s;
    const int64_t lo = ptr[q], len = ptr[q + 1] - lo;
    const int lane = threadIdx.x, ii = lane & 15, kq = lane >> 4;
    const int D = a.D;
    const int u = a.uid[q];
    if ((uint32_t)u >= (uint64_t)a.NU) { *a.err = 1; return; }
    for (int64_t e0 = (int64_t)blockIdx.y * 16; e0 < len; e0 += (int64_t)gridDim.y * 16) {
        int item = e0 + ii < len ? items[lo + e0 + ii] : -1;
        if (item >= 0 && (int64_t)item >= a.NI) { *a.err = 1; item = -1; }
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int kb = 0; kb < a.Dp; kb += 16) {
            float iv[4], uv[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int col = kb + 4 * kq + c;
                iv[c] = (item >= 0 && col < D) ? a.V[(size_t)item * D + col] : 0.0f;
                float v = 0.0f;
                if (col < D) { v = a.U[(size_t)u * D + col]; if (gmf) v *= a.w[col]; }
                uv[c] = v;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(iv[c], uv[c], acc, 0, 0, 0);
        }
        // acc[r] = score(entry e0 + 4 (lane / 16) + r, user column lane % 16)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int it = __shfl(item, 4 * kq + r);
            if (ii == 0 && it >= 0) {
                const float x = acc[r];
                out[lo + e0 + 4 * kq + r] = a.b ? x + a.b[it] : x;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ thresholds ---
// rank_thresholds of kernels_eval.hip into global memory: the chunk's positives sorted by (score, list index)
__global__ __launch_bounds__(64) void evalmf_thresh_kernel(EvalMfArgs a, int c0) {
    __shared__ float raw_s[64];
    __shared__ int raw_ex[64];
    const int NB = a.NB, NT = NB - 1;
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t p0 = a.pos_ptr[q], e0 = a.excl_ptr[q];
    const int n_pos = (int)(a.pos_ptr[q + 1] - p0);
    const int64_t ne = a.excl_ptr[q + 1] - e0;
    const int pc = max(0, min(NT, n_pos - c0));
    float* ts = a.ts + (size_t)q * NB;
    int* tex = a.tex + (size_t)q * NB;
    if (tid < NT) {
        const bool have = tid < pc;
        raw_s[tid] = have ? a.pos_s[p0 + c0 + tid] : INFINITY;
        raw_ex[tid] = have && evalmf_in_sorted(a.excl_items + e0, ne, a.pos_items[p0 + c0 + tid]);
    }
    if (tid == 0) { ts[0] = -INFINITY; tex[NT] = 0; }
    __syncthreads();
    if (tid < NT) {
        const float x = raw_s[tid];
        int r = 0;
        for (int m = 0; m < NT; ++m) r += (raw_s[m] < x) || (raw_s[m] == x && m < tid);
        ts[1 + r] = x; tex[r] = raw_ex[tid];
    }
}

// ------------------------------------------------------------------------------------------ sweep ---
// score_mfma_kernel (kernels_score.hip) with the store replaced by the bucket search.  Everything up to the epilogue is the
// same statement for statement: that is what makes every counted score bit-identical to the scorer's.
template <int KIND, int NSUB, int UW, int KB>
__global__ __launch_bounds__(256) void evalmf_sweep_kernel(EvalMfArgs a, int c0) {
    constexpr int K3 = KIND & 3;
    constexpr bool BIAS = KIND < 4;
    extern __shared__ __attribute__((aligned(16))) float em_lds[];
    const int D = a.D;
    constexpr int Dp = 16 * KB, pitch = Dp + 4;
    constexpr int TI = 16 * NSUB;
    constexpr int UB = 64 * UW;
    float* As = em_lds;
    auto Bsel = [&](int i) -> float* { return em_lds + (UB + i * TI) * pitch; };
    float* un2 = em_lds + (UB + 2 * TI) * pitch;
    float* vn2 = un2 + UB;
    float* bt = vn2 + 2 * TI;
    const int NB = a.NB, tp = NB + 1;                      // (an odd row pitch: users at the same depth of the search sit in different banks)
    float* tsl = bt + 2 * TI;                              // [UB][NB + 1] the users' threshold tables
    unsigned* hl = reinterpret_cast<unsigned*>(tsl + UB * tp);   // [UB][NB + 1] their bucket counters
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q0 = (int64_t)blockIdx.y * UB;
    const int64_t jbeg = (int64_t)blockIdx.x * a.chunk;
    const int64_t jend = jbeg + a.chunk < a.NI ? jbeg + a.chunk : a.NI;
    if (c0 > 0) {                                          // a chunk beyond the positives of every user of this tile
        int any = 0;
        for (int ul = tid; ul < UB; ul += 256)
            if (q0 + ul < a.nq && a.pos_ptr[q0 + ul + 1] - a.pos_ptr[q0 + ul] > c0) any = 1;
        if (!__syncthreads_or(any)) return;
    }
    for (int idx = tid; idx < UB * NB; idx += 256) {
        const int ul = idx / NB, d = idx - ul * NB;
        tsl[ul * tp + d] = q0 + ul < a.nq ? a.ts[(size_t)(q0 + ul) * NB + d] : INFINITY;
        hl[ul * tp + d] = 0u;
    }
    for (int idx = tid; idx < UB * Dp; idx += 256) {
        const int r = idx / Dp, c = idx - r * Dp;
        float v = 0.0f;
        if (q0 + r < a.nq && c < D) {
            const int u = a.uid[q0 + r];
            if ((uint32_t)u >= (uint64_t)a.NU) *a.err = 1;
            else { v = a.U[(size_t)u * D + c]; if (K3 == 2) v *= a.w[c]; }
        }
        As[r * pitch + c] = v;
    }
    const bool vec = (D & 3) == 0;
    const int nv = vec ? (TI * D) / 4 : TI * Dp;
    const int per = (nv + 255) / 256;
    f32x4 stage[8];
    float bstage = 0.f;
    auto fetch = [&](int64_t j0) {
        bstage = (BIAS && tid < TI && j0 + tid < a.NI) ? a.b[j0 + tid] : 0.f;
        if (vec) {
            const f32x4* src = reinterpret_cast<const f32x4*>(a.V + (size_t)j0 * D);
            const int64_t lim = (a.NI - j0) * (int64_t)(D / 4);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int e = tid + 256 * k;
                f32x4 z = {0.f, 0.f, 0.f, 0.f};
                if (k < per && e < nv && e < lim) z = src[e];
                stage[k] = z;
            }
        }
    };
    auto put = [&](float* B, int64_t j0, int buf) {
        if (BIAS && tid < TI) bt[buf * TI + tid] = bstage;
        if (vec) {
            const int q4 = D / 4;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int e = tid + 256 * k;
                if (k < per && e < nv) {
                    const int r = e / q4, c = (e - r * q4) * 4;
                    *reinterpret_cast<f32x4*>(B + r * pitch + c) = stage[k];
                }
            }
        } else {
            for (int idx = tid; idx < TI * Dp; idx += 256) {
                const int r = idx / Dp, c = idx - r * Dp;
                B[r * pitch + c] = (j0 + r < a.NI && c < D) ? a.V[(size_t)(j0 + r) * D + c] : 0.0f;
            }
        }
    };
    if (vec && Dp > D) for (int idx = tid; idx < 2 * TI * (Dp - D); idx += 256) {
        const int r = idx / (Dp - D), c = D + idx % (Dp - D);
        Bsel(0)[r * pitch + c] = 0.0f;
    }
    fetch(jbeg);
    put(Bsel(0), jbeg, 0);
    __syncthreads();
    if (K3 == 1) {
        for (int r = tid; r < UB; r += 256) { float s = 0.f; for (int c = 0; c < Dp; ++c) { const float x = As[r * pitch + c]; s = __builtin_fmaf(x, x, s); } un2[r] = s; }
        if (tid < TI) { const int r = tid; float s = 0.f; for (int c = 0; c < Dp; ++c) { const float x = Bsel(0)[r * pitch + c]; s = __builtin_fmaf(x, x, s); } vn2[r] = s; }
        __syncthreads();
    }
    const float* urow = As + (16 * UW * wave + (lane & 15)) * pitch + 4 * (lane >> 4);
    int t = 0;
    for (int64_t j0 = jbeg; j0 < jend; j0 += TI, ++t) {
        const float* B = Bsel(t & 1);
        const bool more = j0 + TI < jend;
        if (more) fetch(j0 + TI);
        f32x4 acc[UW][NSUB];
#pragma unroll
        for (int g = 0; g < UW; ++g)
#pragma unroll
            for (int s = 0; s < NSUB; ++s) acc[g][s] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* irow = B + (lane & 15) * pitch + 4 * (lane >> 4);
#pragma unroll
        for (int kb = 0; kb < Dp; kb += 16) {
            f32x4 uv[UW], iv[NSUB];
#pragma unroll
            for (int g = 0; g < UW; ++g) uv[g] = *reinterpret_cast<const f32x4*>(urow + g * 16 * pitch + kb);
#pragma unroll
            for (int s = 0; s < NSUB; ++s) iv[s] = *reinterpret_cast<const f32x4*>(irow + s * 16 * pitch + kb);
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int g = 0; g < UW; ++g)
#pragma unroll
                    for (int s = 0; s < NSUB; ++s) acc[g][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(iv[s][c], uv[g][c], acc[g][s], 0, 0, 0);
        }
        // acc[g][s][r] = score(item j0 + 16 s + 4 (lane / 16) + r, user q0 + 16 (UW wave + g) + lane % 16); the epilogue of the
        // scorer's element path, then the bucket search instead of the store
#pragma unroll
        for (int g = 0; g < UW; ++g) {
            const int ul = 16 * (UW * wave + g) + (lane & 15);
            const int64_t q = q0 + ul;
            if (q >= a.nq) continue;
            const float un = K3 == 1 ? un2[ul] : 0.f;
            const float* T = tsl + ul * tp;
            unsigned* H = hl + ul * tp;
#pragma unroll
            for (int s = 0; s < NSUB; ++s) {
                const int64_t j = j0 + 16 * s + 4 * (lane >> 4);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (j + r < jend) {
                        float x = acc[g][s][r];
                        if (K3 == 1) x = 2.0f * x - un - vn2[(t & 1) * TI + 16 * s + 4 * (lane >> 4) + r];
                        const float sc = BIAS ? x + bt[(t & 1) * TI + 16 * s + 4 * (lane >> 4) + r] : x;
                        const int d = evalmf_bucket(T, NB, sc);
                        atomicAdd(&H[d], 1u);
                        if (evalmf_odd(sc, T[d])) {      // rare: exp may round the item onto the threshold below it
                            bool drop;
                            const int c = evalmf_exact(T, sc, d, &drop);
                            if (drop) atomicAdd(&a.nzdrop[q], 1u);
                            for (int m = c; m < d; ++m) atomicAdd(&a.corr[(size_t)q * NB + m], 1u);
                        }
                    }
                }
            }
        }
        if (more) {
            put(Bsel((t + 1) & 1), j0 + TI, (t + 1) & 1);
            if (K3 == 1) {
                __syncthreads();
                if (tid < TI) { float s = 0.f; const float* Bn = Bsel((t + 1) & 1); for (int c = 0; c < Dp; ++c) { const float x = Bn[tid * pitch + c]; s = __builtin_fmaf(x, x, s); } vn2[((t + 1) & 1) * TI + tid] = s; }
            }
        }
        __syncthreads();
    }
    // this run's bucket counts to the users' totals
    for (int idx = tid; idx < UB * NB; idx += 256) {
        const int ul = idx / NB, d = idx - ul * NB;
        const unsigned v = hl[ul * tp + d];
        if (v && q0 + ul < a.nq) atomicAdd(&a.hist[(size_t)(q0 + ul) * NB + d], v);
    }
}

// ------------------------------------------------------------------------------------------ finish ---
// rank_finish_kernel's arithmetic and order; before it, the listed items leave the counts the sweep put them in
__global__ __launch_bounds__(64) void evalmf_finish_kernel(EvalMfArgs a, int c0, int last) {
    __shared__ float T[64];
    __shared__ unsigned sum[64], cr[64], gtp[64];
    __shared__ unsigned nzsub_s, inter_s;
    const int NB = a.NB, NT = NB - 1;
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t p0 = a.pos_ptr[q], e0 = a.excl_ptr[q];
    const int n_pos = (int)(a.pos_ptr[q + 1] - p0);
    const int64_t ne = a.excl_ptr[q + 1] - e0;
    if (c0 == 0 || c0 < n_pos) {
        const int pc = max(0, min(NT, n_pos - c0));
        T[lane] = lane < NB ? a.ts[(size_t)q * NB + lane] : INFINITY;
        sum[lane] = lane < NB ? a.hist[(size_t)q * NB + lane] : 0u;
        cr[lane] = lane < NB ? a.corr[(size_t)q * NB + lane] : 0u;
        gtp[lane] = 0u;
        if (lane == 0) { nzsub_s = 0u; inter_s = 0u; }
        __syncthreads();
        for (int64_t m = lane; m < n_pos + ne; m += 64) {
            const bool isp = m < n_pos;
            const int item = isp ? a.pos_items[p0 + m] : a.excl_items[e0 + (m - n_pos)];
            const float sj = isp ? a.pos_s[p0 + m] : a.excl_s[e0 + (m - n_pos)];
            const bool both = isp ? evalmf_in_sorted(a.excl_items + e0, ne, item) : evalmf_in_sorted(a.pos_items + p0, n_pos, item);
            if (!isp) {                                             // an excluded item is not among the expf > 0 items
                if (both) atomicAdd(&inter_s, 1u);
                if (!(sj < -80.0f && !(expf(sj) > 0.0f))) atomicAdd(&nzsub_s, 1u);
            }
            if (isp || !both) {                                     // each distinct item of P u E once: not an evaluated item
                const int d = evalmf_bucket(T, NB, sj);
                atomicSub(&sum[d], 1u);
                if (evalmf_odd(sj, T[d])) {
                    bool drop;
                    const int c = evalmf_exact(T, sj, d, &drop);
                    for (int k = c; k < d; ++k) atomicSub(&cr[k], 1u);
                }
            }
            // the positives themselves are ranked against too (they are not excluded from rank_above)
            if (isp && !both) {
                const float vm = expf(sj);
                for (int k = 0; k < pc; ++k) if (vm > expf(T[1 + k])) atomicAdd(&gtp[k], 1u);
            }
        }
        __syncthreads();
        if (c0 == 0) {
            if (lane == 0) { a.neval[q] = (int)(a.NI - ((int64_t)n_pos + ne - (int64_t)inter_s)); a.auc[q] = 0.0f; }   // ranking_metrics.py:14
            if (lane < a.nat) { a.ndcg[q * a.nat + lane] = 0.0f; a.recall[q * a.nat + lane] = 0.0f; }
        }
        __syncthreads();
        if (lane == 0 && pc > 0) {                                  // at most 63 positives: one thread, a fixed order of the float sums
            const unsigned nz = (unsigned)a.NI - a.nzdrop[q] - nzsub_s;
            unsigned below = 0, all = 0;
            for (int d = 0; d < NB; ++d) all += sum[d];
            float auc_sum = a.auc[q], nd[16], rc[16];
            for (int t = 0; t < a.nat; ++t) { nd[t] = a.ndcg[q * a.nat + t]; rc[t] = a.recall[q * a.nat + t]; }
            for (int k = 0; k < pc; ++k) {
                below += sum[k];                                    // sum_{d <= k} L[d]
                const unsigned above = a.tex[(size_t)q * NB + k] ? nz : (all - below) - cr[k] + gtp[k];
                auc_sum += (float)below;
                const float g = (float)above;
                const float lr = 1.0f / (logf(g + 2.0f) / logf(2.0f));   // :38 reciprocal(log2(rank_above + 2))
                for (int t = 0; t < a.nat; ++t)
                    if (g < a.at[t]) { nd[t] += lr; rc[t] += 1.0f; }
            }
            a.auc[q] = auc_sum;
            for (int t = 0; t < a.nat; ++t) { a.ndcg[q * a.nat + t] = nd[t]; a.recall[q * a.nat + t] = rc[t]; }
        }
    }
    if (last) {
        __syncthreads();
        if (lane == 0) a.auc[q] = a.auc[q] / ((float)n_pos * (float)a.neval[q]);     // :18-19 (0/0 -> NaN like TF)
        if (lane < a.nat) a.recall[q * a.nat + lane] = a.recall[q * a.nat + lane] / (float)n_pos;   // :62-63
    }
}

// ------------------------------------------------------------------------------------------ launchers ---
int orx_launch_evalmf_gather(orx_ctx* ctx, const EvalMfArgs& a, int kind, int64_t max_list) {
    if (a.nq == 0 || max_list == 0) return ORX_OK;
    ProfScope ps(ctx, ORX_K_GEMM);
    const int64_t tiles = (max_list + 15) / 16;
    ORX_LAUNCH(ctx, evalmf_gather_kernel, dim3((unsigned)a.nq, (unsigned)(tiles < 1024 ? tiles : 1024), 2), dim3(64), 0, a, kind == 2 ? 1 : 0);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

// the sweep's tile: 128 users per workgroup where there are that many and the tables fit the LDS beside the tiles
static int evalmf_uw(int KB, int64_t nq) { return KB <= 4 && nq > 64 ? 2 : 1; }

bool orx_evalmf_has_tile(int D) { return D >= 1 && D <= 128; }

// one chunk of positives of users [0, a.nq): thresholds, sweep over every item, finish
int orx_launch_evalmf_chunk(orx_ctx* ctx, const EvalMfArgs& a_in, int kind, int c0, int last) {
    EvalMfArgs a = a_in;
    if (a.nq == 0) return ORX_OK;
    ORX_ARG(kind == 0 || kind == 2, "evalmf sweep: L2 scores take the dense route");
    ORX_ARG(orx_evalmf_has_tile(a.D), "evalmf sweep: no tile for dim %d", a.D);
    int KB = 1;
    while (16 * KB < a.D) KB *= 2;
    a.Dp = 16 * KB;
    const int pitch = a.Dp + 4;
    const int UW = evalmf_uw(KB, a.nq);
    const int TI = 64;
    a.TI = TI;
    const int64_t nqt = (a.nq + 64 * UW - 1) / (64 * UW);
    // items per workgroup: about 1024 workgroups; a run never so short that loading and flushing the tables dominates it
    int64_t chunk = (a.NI * nqt + 1023) / 1024;
    chunk = ((chunk + TI - 1) / TI) * TI;
    if (chunk < 16 * TI) chunk = 16 * TI;
    a.chunk = chunk;
    const size_t lds = ((size_t)(64 * UW + 2 * TI) * pitch + 64 * UW + 4 * TI + (size_t)2 * 64 * UW * (a.NB + 1)) * sizeof(float);
    const dim3 g((unsigned)((a.NI + chunk - 1) / chunk), (unsigned)nqt);
    ORX_HIP(hipMemsetAsync(a.hist, 0, (size_t)a.nq * a.NB * 2 * sizeof(unsigned), ctx->stream));      // hist | corr
    ORX_HIP(hipMemsetAsync(a.nzdrop, 0, (size_t)a.nq * sizeof(unsigned), ctx->stream));
    ORX_LAUNCH(ctx, evalmf_thresh_kernel, dim3((unsigned)a.nq), dim3(64), 0, a, c0);
#define ORX_EM(K, N, W, B) do { \
        ORX_ONCE_PER_DEVICE(ctx, ORX_HIP(hipFuncSetAttribute((const void*)evalmf_sweep_kernel<K, N, W, B>, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024))); \
        ProfScope ps(ctx, ORX_K_GEMM); \
        ORX_LAUNCH(ctx, (evalmf_sweep_kernel<K, N, W, B>), g, dim3(256), lds, a, c0); } while (0)
#define ORX_EMW(K, B) do { if (UW == 2) ORX_EM(K, 4, 2, B); else ORX_EM(K, 4, 1, B); } while (0)
#define ORX_EMK(K) do { switch (KB) { case 1: ORX_EMW(K, 1); break; case 2: ORX_EMW(K, 2); break; case 4: ORX_EMW(K, 4); break; \
                                      default: ORX_EM(K, 4, 1, 8); break; } } while (0)
    if (a.b == nullptr) {
        if (kind == 0) ORX_EMK(4); else ORX_EMK(6);
    } else if (kind == 0) ORX_EMK(0); else ORX_EMK(2);
#undef ORX_EMK
#undef ORX_EMW
#undef ORX_EM
    ORX_LAUNCH(ctx, evalmf_finish_kernel, dim3((unsigned)a.nq), dim3(64), 0, a, c0, last);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}
