// Top-K recommendation on the device (orx_recommend_topk, orx_topk_rows) without an [n, items] score matrix.
//
// Semantics.  For user q and item j the score s(q, j) is exactly what orx_score_all_items returns (bit for bit, default
// build).  The result of a row is the k ELIGIBLE items with the largest scores, ordered by score descending and then by
// item id ascending (tf.math.top_k's tie rule: the lower index first).  An item is not eligible when it is in the user's
// exclusion list or its score is NaN; -inf is an ordinary score.  A row with fewer than k eligible items is filled up
// with item -1 / score -inf.  The selection is a function of the (score, id) set alone: no launch shape, arrival order
// or atomic decides anything, so a call repeated gives the same bits.
//
// Fused route (MFMA tiles, D <= 256), per batch of users:
//   1. threshold  the exact k-th best eligible score theta_q over the first P items (the normal scorer into [nb, P]
//                 scratch, then topk_select_kernel in threshold mode).  At least k eligible items score >= theta_q, so
//                 the top k over ALL items all do.  Fewer than k eligible sample items: the user goes to step 4.
//   2. filter     topk_filter_kernel: the MFMA tile product of score_mfma_kernel (restated below: the same operand layout,
//                 k order and epilogue arithmetic, hence the same bits) over every item; a score >= theta_q goes into the
//                 workgroup's pool (an LDS atomic and two stores), and every 8 tiles a pool half full -- and the pool at the
//                 end -- is appended to the users' candidate lists of capacity C with one global atomic per user.  Nothing
//                 is stored per score.
//   3. select     topk_select_kernel over each user's candidates, one workgroup per user, excluded items skipped (binary
//                 search in the user's sorted exclusion row, in LDS): an MSB-first radix select of the k-th key (8-bit
//                 digits), a second one over the ids of the keys tied with it, then a bitonic sort of the k winners in LDS
//                 by (score desc, id asc).
//   4. fallback   a user whose candidates overflowed C is scored row by row into bounded scratch with the normal scorer
//                 and selected by the same kernel over the dense row (what orx_topk_rows does).  Many equal scores (a
//                 constant table, identical item rows) land here and stay exact.
// UCML (L2) scores take step 4's route for every user: their |u|^2 and |v|^2 sums were fp32 chains in which the compiler fused
// some products into FMAs and rounded others (a choice made per kernel body), so a restated kernel did not reproduce the
// scorer's bits from the same source.  The sums are explicit fmaf chains now (kernels_score.hip says why), here as there; the
// L2 branches of the restated kernel below stay statement for statement the scorer's, but they are still not instantiated.
// D > 256 (no MFMA tile), ORX_SCORE_SIMPLE, and item counts no larger than the sample take step 4's route directly, in
// bounded user batches.  Device scratch: nb x (P + 2 C + 2 k) words per batch of nb users, the pools (TOPK_FILTER_BLOCKS x
// TOPK_POOL x 12 bytes: a longer item table gets longer chunks, not more workgroups) and at most ORX_TOPK_DENSE_BYTES of dense
// rows; P grows with k items / C, nothing else with the item count.
#include "orx_device.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------- ordering keys ---
// An unsigned key whose order is the score order; -0 is folded into +0 (they compare equal, so the id decides).
__device__ __forceinline__ uint32_t topk_key(float s) {
    uint32_t u = __float_as_uint(s);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float topk_key_score(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// is `id` in the sorted list e[0 .. ne)?
__device__ __forceinline__ bool topk_in_sorted(const int32_t* e, int64_t ne, int32_t id) {
    int64_t lo = 0, hi = ne;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (e[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo < ne && e[lo] == id;
}

// ------------------------------------------------------------------------------------------ filter kernel ---
struct TopkFilterArgs {
    const float* U; const float* V; const float* b; const float* w;
    const int32_t* uid; int64_t nq; int64_t NU; int64_t NI;
    int D; int Dp; int TI; int64_t chunk;
    const float* theta;                         // [nq] the users' thresholds (NaN: no candidates, the user is redone densely)
    int* cnt; float* cs; int32_t* ci; int C;    // [nq] candidate counts, [nq][C] candidate scores / ids
    int2* pool_iu; float* pool_s; int pool_cap; // [workgroups][pool_cap] the workgroup's pending candidates: (item, user slot), score
    int* err;
};

// score_mfma_kernel (kernels_score.hip) with the store replaced by the threshold test.  Everything up to the epilogue is
// the same statement for statement: that is what makes every emitted score bit-identical to the scorer's.
template <int KIND, int NSUB, int UW, int KB>
__global__ __launch_bounds__(256) void topk_filter_kernel(TopkFilterArgs a) {
    constexpr int K3 = KIND & 3;
    constexpr bool BIAS = KIND < 4;
    extern __shared__ __attribute__((aligned(16))) float tf_lds[];
    const int D = a.D;
    constexpr int Dp = 16 * KB, pitch = Dp + 4;
    constexpr int TI = 16 * NSUB;
    constexpr int UB = 64 * UW;
    float* As = tf_lds;
    auto Bsel = [&](int i) -> float* { return tf_lds + (UB + i * TI) * pitch; };
    float* un2 = tf_lds + (UB + 2 * TI) * pitch;
    float* vn2 = un2 + UB;
    float* bt = vn2 + 2 * TI;
    int* pend = reinterpret_cast<int*>(bt + 2 * TI);      // [1] pending candidates in the pool
    int* ucnt = pend + 1;                                  // [UB] per user slot: candidates of a flush
    int* ubase = ucnt + UB;                                // [UB] their first position in the user's list
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q0 = (int64_t)blockIdx.y * UB;
    const int64_t jbeg = (int64_t)blockIdx.x * a.chunk;
    const int64_t jend = jbeg + a.chunk < a.NI ? jbeg + a.chunk : a.NI;
    const size_t pbase = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * a.pool_cap;
    if (tid == 0) *pend = 0;
    for (int i = tid; i < UB; i += 256) ucnt[i] = 0;
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
    // the pool to the users' lists: one global atomic per user slot and flush (called by all threads behind a barrier)
    auto flush = [&]() {
        const int raw = *pend, n = raw < a.pool_cap ? raw : a.pool_cap;
        if (raw > a.pool_cap)                              // candidates were dropped: these users are redone densely
            for (int ul = tid; ul < UB; ul += 256) if (q0 + ul < a.nq) atomicMax(a.cnt + q0 + ul, 1 << 30);
        for (int i = tid; i < n; i += 256) atomicAdd(&ucnt[a.pool_iu[pbase + i].y], 1);
        __syncthreads();
        for (int ul = tid; ul < UB; ul += 256) {
            const int c = ucnt[ul];
            ubase[ul] = c ? atomicAdd(a.cnt + q0 + ul, c) : 0;
            ucnt[ul] = 0;
        }
        __syncthreads();
        for (int i = tid; i < n; i += 256) {
            const int2 e = a.pool_iu[pbase + i];
            const int pos = ubase[e.y] + atomicAdd(&ucnt[e.y], 1);
            if (pos < a.C) { a.cs[(size_t)(q0 + e.y) * a.C + pos] = a.pool_s[pbase + i]; a.ci[(size_t)(q0 + e.y) * a.C + pos] = e.x; }
        }
        __syncthreads();
        for (int ul = tid; ul < UB; ul += 256) ucnt[ul] = 0;
        if (tid == 0) *pend = 0;
        __syncthreads();
    };
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
    // the thresholds of this lane's users, once
    float th[UW];
#pragma unroll
    for (int g = 0; g < UW; ++g) {
        const int64_t q = q0 + 16 * (UW * wave + g) + (lane & 15);
        th[g] = q < a.nq ? a.theta[q] : __builtin_nanf("");
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
        // scorer's element path, then the threshold test instead of the store
#pragma unroll
        for (int g = 0; g < UW; ++g) {
            const int ul = 16 * (UW * wave + g) + (lane & 15);
            const int64_t q = q0 + ul;
            if (q >= a.nq) continue;
            const float un = K3 == 1 ? un2[ul] : 0.f;
#pragma unroll
            for (int s = 0; s < NSUB; ++s) {
                const int64_t j = j0 + 16 * s + 4 * (lane >> 4);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (j + r < jend) {
                        float x = acc[g][s][r];
                        if (K3 == 1) x = 2.0f * x - un - vn2[(t & 1) * TI + 16 * s + 4 * (lane >> 4) + r];
                        const float sc = BIAS ? x + bt[(t & 1) * TI + 16 * s + 4 * (lane >> 4) + r] : x;
                        if (sc >= th[g]) {               // rare: into the workgroup's pool (an LDS atomic, no global round trip)
                            const int slot = atomicAdd(pend, 1);
                            if (slot < a.pool_cap) { a.pool_iu[pbase + slot] = make_int2((int)(j + r), ul); a.pool_s[pbase + slot] = sc; }
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
        if ((t & 7) == 7) {                      // every 8 tiles: a pool half full is emptied (the count is read before anyone adds again)
            const int now = *pend;
            __syncthreads();
            if (now > a.pool_cap / 2) flush();
        }
    }
    flush();
}

// the tile shapes of orx_launch_score_mfma; returns ORX_OK and *launched = false where the scorer has no MFMA tile either
int orx_launch_topk_filter(orx_ctx* ctx, const float* U, const float* V, const float* b, const float* w, const int32_t* uid,
                           int64_t nq, int64_t NU, int64_t NI, int D, int kind, const float* theta, int* cnt, float* cs,
                           int32_t* ci, int C, int2* pool_iu, float* pool_s, bool* launched) {
    *launched = false;
    int KB = 1;
    while (16 * KB < D) KB *= 2;
    if (KB > 16) return ORX_OK;
    TopkFilterArgs a;
    a.U = U; a.V = V; a.b = b; a.w = w; a.uid = uid; a.nq = nq; a.NU = NU; a.NI = NI; a.D = D; a.Dp = 16 * KB;
    a.theta = theta; a.cnt = cnt; a.cs = cs; a.ci = ci; a.C = C; a.err = ctx->d_err;
    a.pool_iu = pool_iu; a.pool_s = pool_s; a.pool_cap = TOPK_POOL;
    const int pitch = a.Dp + 4;
    const int UW = KB == 16 ? 1 : (nq > 64 ? 2 : 1);
    const int TI = KB == 16 ? 32 : 64;
    a.TI = TI;
    const int64_t nqt = (nq + 64 * UW - 1) / (64 * UW);
    int64_t chunk = (NI * nqt + 1023) / 1024;
    chunk = ((chunk + TI - 1) / TI) * TI;
    if (chunk < 4 * TI) chunk = 4 * TI;
    if (chunk > 4096) chunk = 4096;
    ORX_ARG(nqt <= TOPK_FILTER_BLOCKS, "topk filter: %lld user groups", (long long)nqt);
    const int64_t gx_max = TOPK_FILTER_BLOCKS / nqt;       // (the pools are sized for TOPK_FILTER_BLOCKS workgroups, whatever the items)
    if ((NI + chunk - 1) / chunk > gx_max) chunk = ((NI + gx_max - 1) / gx_max + TI - 1) / TI * TI;
    a.chunk = chunk;
    const size_t lds = ((size_t)(64 * UW + 2 * TI) * pitch + 64 * UW + 4 * TI) * sizeof(float) + (1 + 2 * 64 * UW) * sizeof(int);
    const dim3 g((unsigned)((NI + chunk - 1) / chunk), (unsigned)nqt);
    ProfScope ps(ctx, ORX_K_GEMM);
#define ORX_TF(K, N, W, B) do { \
        ORX_ONCE_PER_DEVICE(ctx, ORX_HIP(hipFuncSetAttribute((const void*)topk_filter_kernel<K, N, W, B>, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024))); \
        ORX_LAUNCH(ctx, (topk_filter_kernel<K, N, W, B>), g, dim3(256), lds, a); } while (0)
#define ORX_TFW(K, B) do { if (UW == 2) ORX_TF(K, 4, 2, B); else ORX_TF(K, 4, 1, B); } while (0)
#define ORX_TFK(K) do { switch (KB) { case 1: ORX_TFW(K, 1); break; case 2: ORX_TFW(K, 2); break; case 4: ORX_TFW(K, 4); break; \
                                      case 8: ORX_TFW(K, 8); break; default: ORX_TF(K, 2, 1, 16); break; } } while (0)
    ORX_ARG(kind != 1, "topk filter: L2 scores take the dense route");
    if (b == nullptr) {
        if (kind == 0) ORX_TFK(4); else ORX_TFK(6);
    } else if (kind == 0) ORX_TFK(0); else ORX_TFK(2);
#undef ORX_TFK
#undef ORX_TFW
#undef ORX_TF
    ORX_HIP(hipGetLastError());
    *launched = true;
    return ORX_OK;
}

// ------------------------------------------------------------------------------------------ select kernel ---
constexpr int TOPK_KMAX = 1024;     // largest k
constexpr int TOPK_ECACHE = 2048;   // exclusion rows up to this long are searched in LDS


__global__ __launch_bounds__(256) void topk_select_kernel(TopkSelectArgs a) {
    __shared__ int hist[256];
    __shared__ uint32_t skey[TOPK_KMAX];
    __shared__ int32_t sid[TOPK_KMAX];
    __shared__ float ssc[TOPK_KMAX];
    __shared__ int32_t ecache[TOPK_ECACHE];
    __shared__ int s_sel, s_cum, s_tie, s_n;
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int64_t q = a.rowmap ? a.rowmap[r] : r;
    const bool cand = a.cs != nullptr;
    int64_t n;
    if (cand) {
        const int c = a.cnt[q];
        if (c > a.C) return;
        n = c;
    } else n = a.m;
    int64_t ne = 0;
    const int32_t* erow = nullptr;
    if (a.eptr) { erow = a.eitems + a.eptr[q]; ne = a.eptr[q + 1] - a.eptr[q]; }
    if (ne <= TOPK_ECACHE) {
        for (int64_t i = tid; i < ne; i += 256) ecache[i] = erow[i];
        erow = ecache;
    }
    __syncthreads();
    // (score, id, eligible) of element i
    auto load = [&](int64_t i, float& s, int32_t& id) -> bool {
        if (cand) { s = a.cs[(size_t)q * a.C + i]; id = a.ci[(size_t)q * a.C + i]; return true; }
        s = a.scores[(size_t)r * a.ld + i]; id = (int32_t)i;
        return !__builtin_isnan(s);
    };
    auto excluded = [&](int32_t id) -> bool { return ne != 0 && topk_in_sorted(erow, ne, id); };

    // 1. the k-th largest key: 8 bits at a time from the top
    uint32_t prefix = 0u, pmask = 0u;
    int need = a.k;
    bool all = false;                      // fewer than k eligible: every one of them is taken
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = tid; i < 256; i += 256) hist[i] = 0;
        __syncthreads();
        for (int64_t i = tid; i < n; i += 256) {
            float s; int32_t id;
            if (!load(i, s, id)) continue;
            const uint32_t key = topk_key(s);
            if ((key & pmask) != prefix || excluded(id)) continue;
            atomicAdd(&hist[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int c = 0, sel = -1;
            for (int bin = 255; bin >= 0; --bin) {
                if (c + hist[bin] >= need) { sel = bin; break; }
                c += hist[bin];
            }
            s_sel = sel; s_cum = c; s_tie = sel >= 0 ? hist[sel] : 0;
        }
        __syncthreads();
        const int sel = s_sel, cum = s_cum;
        if (sel < 0) { all = true; break; }          // (only in the first pass: later ones stay inside a bin that holds >= need)
        need -= cum;
        prefix |= (uint32_t)sel << shift;
        pmask |= 0xffu << shift;
    }
    const uint32_t T = prefix;
    if (a.theta) {
        if (tid == 0) {
            a.theta[q] = all ? __builtin_nanf("") : topk_key_score(T);
            a.cnt[q] = all ? a.C + 1 : 0;
        }
        return;
    }
    // 2. of the keys equal to T, the `need` smallest ids: the largest id taken
    uint32_t idmax = 0xffffffffu;
    if (!all && need < s_tie) {
        uint32_t ip = 0u, im = 0u;
        int need2 = need;
        for (int shift = 24; shift >= 0; shift -= 8) {
            __syncthreads();
            for (int i = tid; i < 256; i += 256) hist[i] = 0;
            __syncthreads();
            for (int64_t i = tid; i < n; i += 256) {
                float s; int32_t id;
                if (!load(i, s, id) || topk_key(s) != T || ((uint32_t)id & im) != ip || excluded(id)) continue;
                atomicAdd(&hist[((uint32_t)id >> shift) & 255u], 1);
            }
            __syncthreads();
            if (tid == 0) {
                int c = 0, sel = 255;
                for (int bin = 0; bin < 256; ++bin) {
                    if (c + hist[bin] >= need2) { sel = bin; break; }
                    c += hist[bin];
                }
                s_sel = sel; s_cum = c;
            }
            __syncthreads();
            need2 -= s_cum;
            ip |= (uint32_t)s_sel << shift;
            im |= 0xffu << shift;
        }
        idmax = ip;
    }
    // 3. gather the winners (at most k) and sort them by (score desc, id asc)
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int64_t i = tid; i < n; i += 256) {
        float s; int32_t id;
        if (!load(i, s, id)) continue;
        const uint32_t key = topk_key(s);
        if (!(all || key > T || (key == T && (uint32_t)id <= idmax)) || excluded(id)) continue;
        const int slot = atomicAdd(&s_n, 1);
        skey[slot] = key; sid[slot] = id; ssc[slot] = s;
    }
    __syncthreads();
    const int cntk = s_n;
    int NS = 1;
    while (NS < cntk) NS <<= 1;
    for (int i = cntk + tid; i < NS; i += 256) { skey[i] = 0u; sid[i] = 0x7fffffff; }     // below every real key (NaN is never one)
    __syncthreads();
    for (int size = 2; size <= NS; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int p = tid; p < NS / 2; p += 256) {
                const int i = 2 * p - (p & (stride - 1)), j = i + stride;
                const bool j_first = skey[j] > skey[i] || (skey[j] == skey[i] && sid[j] < sid[i]);
                if (j_first == ((i & size) == 0)) {
                    const uint32_t tk = skey[i]; skey[i] = skey[j]; skey[j] = tk;
                    const int32_t ti = sid[i]; sid[i] = sid[j]; sid[j] = ti;
                    const float ts = ssc[i]; ssc[i] = ssc[j]; ssc[j] = ts;
                }
            }
            __syncthreads();
        }
    }
    int32_t* oi = a.out_items + (size_t)q * a.k;
    float* os = a.out_scores + (size_t)q * a.k;
    for (int i = tid; i < a.k; i += 256) {
        oi[i] = i < cntk ? sid[i] : -1;
        os[i] = i < cntk ? ssc[i] : -__builtin_inff();
    }
}

int orx_launch_topk_select(orx_ctx* ctx, const TopkSelectArgs& a, int64_t rows) {
    if (rows == 0) return ORX_OK;
    ProfScope ps(ctx, ORX_K_GEMM);
    ORX_LAUNCH(ctx, topk_select_kernel, dim3((unsigned)rows), dim3(256), 0, a);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}
