// Exact top-K through a bf16 matrix-core prefilter (orx_recommend_topk with ORX_TOPK_BF16_PREFILTER; kernels_topk.hip has the
// semantics, which this route does not change by one bit; DESIGN 4.5c.1 has the derivation and the measurements).
//
// Per call   topk16_items_kernel: V16 [NIp][Dk], the round-to-nearest-even bf16 copy of the item rows (Dk = D rounded up to 32, NIp =
//            items rounded up to 64, zeros in the padding), and two floats per item: nrm[j], an upper bound B_j of |v_j| (dot, GMF) or
//            the scorer's |v_j|^2 chain (L2: its bits), and hg[j], the item's side of the test below.
// Per batch  thresholds as in the fp32 route (theta_q: the exact k-th best eligible fp32 score of the first P items), then
//   topk16_filter_kernel   s16 = bf(x_q) . bf(v_j) for every (user, item) on v_mfma_f32_16x16x32_bf16, and the pair is DROPPED only
//                          when s16 plus the margin M_qj below is under theta_q; whatever is kept goes to the user's candidate list as
//                          an item id alone.  Kept: a superset of {j : s(q, j) >= theta_q}.
//   topk16_rescore_kernel  every candidate gets the scorer's own fp32 score (the MFMA construction of cand_score_kernel, restated
//                          and extended to dim 256 and to L2), the exact test s >= theta_q of topk_filter_kernel is applied, and the
//                          survivors are compacted in place into (cs, ci, cnt): the very candidate SET the fp32 filter leaves.
//   then topk_select_kernel and the dense fallback of overflowed users, unchanged.
//
// The margin.  x: the user operand as the scorer rounds it (u, or fl(u w) for GMF), y = v_j, A = |x|_2, B = |y|_2, d = sum x_c y_c.
//   operands   RNE bf16: bf(x_c) = x_c (1 + e), |e| <= 2^-8, so |bf(x_c) bf(y_c) - x_c y_c| <= (2^-7 + 2^-16) |x_c y_c|, and the
//              bf16 products are exact in fp32.  Summed, with Cauchy-Schwarz: <= (2^-7 + 2^-16) A B.
//   sums       either fp32 accumulation (the scorer's over Dp terms, this one over Dk) is off by at most 2^-23 per addition of the
//              sum of the absolute products, in any order: together <= (Dp + Dk) 2^-23 1.01 A B <= Dk 2^-21 A B.
//   so         |d16 - d32| <= c0 A B with c0 = 2^-7 + 2^-16 + Dk 2^-21; the kernel uses c = 1.05 2^-7 + Dk 2^-20 >= c0 + 2^-12.
//   epilogue   dot / GMF add b_j, L2 forms (2 d - un) - vn + b_j: at most 3 fp32 roundings in the scorer and 5 in the test here, each
//              <= 2^-24 of a magnitude <= G = 2.04 A B + un + vn + 1.01 |b_j|, in total <= 2^-21 G.  The test carries 2^-18 (|b_j| + vn)
//              on the item side, 2^-18 un on the user side and the 2^-12 A B (twice that for L2) left in c.
//   tiny       operands under 2^-126 may be flushed or rounded absolutely, products under 2^-126 too: at most 2^-121 (A + B) + 2^-117.
//              The test carries 2^-100 (A + B) and 2e-37; A and B are rounded up and carry + 2^-59 for squares that underflowed.
//   rounding   a slack term smaller than half an ulp of what it is added to would vanish: the item side is stepped UP by up(), the
//              user side DOWN by down() (a relative 2^-22 and 1e-37), after which monotone rounding keeps every inequality.
//   non-finite A or B above 2^60 (or NaN) counts as infinite: then no partial sum of finite operands can overflow.  An infinite or
//              NaN B_j makes T NaN or +inf: kept.  A user whose A is not finite is marked for the dense fallback, as one whose
//              theta is NaN (fewer than k eligible sample items) already is.  b_j = -inf gives s = -inf exactly: dropped unless
//              theta_q is -inf.  "Drop iff T < thl" keeps every NaN.
// The test, three VALU operations per score:   t = s16 + hg_j  (L2: 2 s16 + hg_j, hg_j holding b_j - vn_j);
//   T = fma(cA_q, B_j, t);   drop iff T < thl_q,   thl_q = down(theta_q [+ un_q] - slack_q).
//
// Data path of the filter.  A workgroup owns 64 UW users, UW in {1, 2, 4} from D and the user count: wavefront w UW groups of 16, whose
// rows never touch LDS -- lane (ln, q) keeps k = 8 q .. 8 q + 7 of every k-block of 32 of user row ln as one bf16x8 B operand for the
// whole walk (GMF: times w in fp32 first).  It walks its chunk of V16 in tiles of 64 rows: the next tile's 16-byte global loads are in
// flight under the current tile's products and land row-major in the other half of a double-buffered LDS tile (pitch 2 Dk + 16 bytes:
// ds_read_b128 without bank conflicts), with the tile's hg_j and B_j beside it; one barrier per tile.  4 UW MFMAs per k-block feed
// 4 UW interleaved accumulators; lane (ln, q) ends with items 16 s + 4 q + r of user ln, reads hg and B as two ds_read_b128 per s.
// Pool, flushes, per-user atomics, capacity C and the overflow marking are topk_filter_kernel's, without the scores; the pool is
// looked at after every tile, by one thread ahead of the tile's barrier.
#include <algorithm>

#include "orx_device.h"
#include "orx_mfma16.h"

namespace {

constexpr float T16_REL = 0x1p-18f;          // relative slack for the epilogue roundings
constexpr float T16_TINY = 0x1p-100f;        // times (A + B): flushed subnormals
constexpr float T16_BIG = 0x1p60f;           // a norm above this counts as infinite

__device__ __forceinline__ float t16_up(float x) { return __builtin_fmaf(__builtin_fabsf(x), 0x1p-22f, x) + 1e-37f; }
__device__ __forceinline__ float t16_down(float x) { return __builtin_fmaf(-__builtin_fabsf(x), 0x1p-22f, x) - 1e-37f; }
// an upper bound of sqrt(the exact sum of squares) from its fp32 sum `ss` over at most `terms` terms
__device__ __forceinline__ float t16_norm(float ss, int terms) {
    const float n = __builtin_sqrtf(ss * (1.0f + (float)terms * 0x1p-22f)) * (1.0f + 0x1p-12f) + 0x1p-59f;
    return n <= T16_BIG ? n : __builtin_inff();       // (NaN too)
}

__device__ __forceinline__ u32x4 t16_pack(const float (&x)[8]) {
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (__bf16)x[j];
    return __builtin_bit_cast(u32x4, v);
}

// ------------------------------------------------------------------------------------------ item copy ---
constexpr int T16_IR = 32;       // item rows per workgroup

__global__ __launch_bounds__(256) void topk16_items_kernel(Topk16ItemArgs a) {
    extern __shared__ __attribute__((aligned(16))) float t16_rows[];       // [T16_IR][D + 1]
    const int D = a.D, Dk = a.Dk, lp = D + 1, tid = threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * T16_IR;
    const int64_t have = a.NI - j0 < T16_IR ? (a.NI - j0 > 0 ? a.NI - j0 : 0) : T16_IR;   // rows of this tile that exist
    if ((D & 3) == 0) {
        const f32x4* src = reinterpret_cast<const f32x4*>(a.V + (size_t)j0 * D);
        const int q4 = D >> 2;
        for (int e = tid; e < T16_IR * q4; e += 256) {
            const int r = e / q4, c = (e - r * q4) * 4;
            const f32x4 z = r < have ? src[e] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 4; ++i) t16_rows[r * lp + c + i] = z[i];
        }
    } else {
        for (int e = tid; e < T16_IR * D; e += 256) {
            const int r = e / D, c = e - r * D;
            t16_rows[r * lp + c] = r < have ? a.V[(size_t)j0 * D + e] : 0.0f;
        }
    }
    __syncthreads();
    const int g8 = Dk >> 3;
    for (int e = tid; e < T16_IR * g8; e += 256) {
        const int r = e / g8, c = 8 * (e - r * g8);
        float x[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = c + i < D ? t16_rows[r * lp + c + i] : 0.0f;
        *reinterpret_cast<u32x4*>(a.V16 + (size_t)(j0 + r) * Dk + c) = t16_pack(x);
    }
    if (tid < T16_IR) {
        const int64_t j = j0 + tid;
        // the scorer's |v|^2 chain (kernels_score.hip): its padding columns add fmaf(0, 0, s) = s, so they are left out
        float s = 0.f;
        for (int c = 0; c < D; ++c) { const float x = t16_rows[tid * lp + c]; s = __builtin_fmaf(x, x, s); }
        float nrm = 0.f, hg = 0.f;
        if (j < a.NI) {
            const float B = t16_norm(s, D);
            const float bj = a.b ? a.b[j] : 0.0f;
            const float base = a.l2 ? bj - s : bj;
            const float slack = __builtin_fmaf(T16_REL, __builtin_fabsf(bj) + (a.l2 ? s : 0.0f), T16_TINY * B);
            hg = base == -__builtin_inff() ? base : t16_up(base + slack);
            nrm = a.l2 ? s : B;
        }
        a.nrm[j] = nrm; a.hg[j] = hg;
    }
}

// --------------------------------------------------------------------------------------------- filter ---
template <bool L2, int UW, int KBMAX>
__global__ __launch_bounds__(256) void topk16_filter_kernel(Topk16FilterArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char t16_lds[];
    constexpr int UB = 64 * UW;
    const int D = a.D, Dk = a.Dk, nkb = Dk >> 5, pitch = 2 * Dk + 16, c8n = Dk >> 3;
    unsigned char* Bs = t16_lds;                                              // [2][64][pitch bytes] the item tiles, row-major
    float* th = reinterpret_cast<float*>(Bs + 2 * 64 * pitch);                // [2][64] hg_j
    float* tb = th + 128;                                                     // [2][64] B_j
    int* pend = reinterpret_cast<int*>(tb + 128);                             // [1] pending candidates in the pool
    int* ucnt = pend + 1;                                                     // [UB] per user slot: candidates of a flush
    int* ubase = ucnt + UB;                                                   // [UB] their first position in the user's list
    int* full = ubase + UB;                                                   // [2] "the pool is half full", per tile parity
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, ln = lane & 15;
    const int64_t q0 = (int64_t)blockIdx.y * UB;
    const int64_t jbeg = (int64_t)blockIdx.x * a.chunk;
    const int64_t jend = jbeg + a.chunk < a.NIp ? jbeg + a.chunk : a.NIp;     // whole tiles: chunk and NIp are multiples of 64
    const size_t pbase = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * a.pool_cap;
    if (tid == 0) *pend = 0;
    for (int i = tid; i < UB; i += 256) ucnt[i] = 0;

    // this lane's users: the bf16 operand fragments, cA_q and the lowered threshold (NaN: the user is skipped)
    bf16x8 ov[UW][KBMAX];
    float cA[UW], thl[UW];
#pragma unroll
    for (int g = 0; g < UW; ++g) {
        const int64_t qg = q0 + 16 * (UW * wave + g) + ln;
        bool valid = qg < a.nq;
        int u = 0;
        if (valid) {
            u = a.uid[qg];
            if ((uint32_t)u >= (uint64_t)a.NU) { *a.err = 1; valid = false; }
        }
        const float* urow = a.U + (size_t)u * D;
        float ss = 0.f;
#pragma unroll
        for (int kb = 0; kb < KBMAX; ++kb) {
            float x[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int c = 32 * kb + 8 * q + i;
                float v = 0.0f;
                if (valid && kb < nkb && c < D) { v = urow[c]; if (a.gmf) v *= a.w[c]; }
                x[i] = v;
                ss = __builtin_fmaf(v, v, ss);
            }
            ov[g][kb] = __builtin_bit_cast(bf16x8, t16_pack(x));
        }
        ss += __shfl_xor(ss, 16);
        ss += __shfl_xor(ss, 32);
        float un = 0.f;
        if (L2) {                                        // the scorer's |u|^2 chain, by the lane group q = 0
            if (valid && q == 0) for (int c = 0; c < D; ++c) { const float x = urow[c]; un = __builtin_fmaf(x, x, un); }
            un = __shfl(un, ln);
        }
        const float A = t16_norm(ss, Dk);
        const float theta = valid ? a.theta[qg] : __builtin_nanf("");
        float lo = __builtin_nanf("");
        if (theta == theta) {
            if (A < __builtin_inff()) lo = t16_down((L2 ? theta + un : theta) - __builtin_fmaf(T16_REL, un, T16_TINY * A));
            if (lo != lo && q == 0) atomicMax(a.cnt + qg, 1 << 30);  // A or theta + un not finite: this user is redone densely
        }
        thl[g] = lo;
        cA[g] = (L2 ? 2.0f : 1.0f) * a.cmul * A;
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
            if (pos >= 0 && pos < a.C) a.ci[(size_t)(q0 + e.y) * a.C + pos] = e.x;
        }
        __syncthreads();
        for (int ul = tid; ul < UB; ul += 256) ucnt[ul] = 0;
        if (tid == 0) *pend = 0;
        __syncthreads();
    };

    u32x4 stage[KBMAX];
    float sside = 0.f;
    auto fetch = [&](int64_t j0) {
        const u32x4* src = reinterpret_cast<const u32x4*>(a.V16 + (size_t)j0 * Dk);     // 64 c8n = 256 nkb groups of eight, contiguous
#pragma unroll
        for (int k = 0; k < KBMAX; ++k)
            if (k < nkb) stage[k] = src[tid + 256 * k];
        if (tid < 64) sside = a.hg[j0 + tid];
        else if (tid < 128) sside = a.nrm[j0 + tid - 64];
    };
    auto put = [&](int buf) {
        unsigned char* B = Bs + buf * 64 * pitch;
#pragma unroll
        for (int k = 0; k < KBMAX; ++k)
            if (k < nkb) {
                const int e = tid + 256 * k, r = e / c8n, c = e - r * c8n;
                *reinterpret_cast<u32x4*>(B + r * pitch + 16 * c) = stage[k];
            }
        if (tid < 64) th[buf * 64 + tid] = sside;
        else if (tid < 128) tb[buf * 64 + tid - 64] = L2 ? t16_norm(sside, D) : sside;
    };

    fetch(jbeg);
    put(0);
    __syncthreads();
    int t = 0;
    for (int64_t j0 = jbeg; j0 < jend; j0 += 64, ++t) {
        const int cur = t & 1;
        const bool more = j0 + 64 < jend;
        if (more) fetch(j0 + 64);
        f32x4 acc[UW][4];
#pragma unroll
        for (int g = 0; g < UW; ++g)
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[g][s] = f32x4{0.f, 0.f, 0.f, 0.f};
        const unsigned char* wrow = Bs + cur * 64 * pitch + ln * pitch + 16 * q;
#pragma unroll
        for (int kb = 0; kb < KBMAX; ++kb) {
            if (kb < nkb) {
                bf16x8 wv[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) wv[s] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(wrow + s * 16 * pitch + 64 * kb));
#pragma unroll
                for (int g = 0; g < UW; ++g)
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc[g][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv[s], ov[g][kb], acc[g][s], 0, 0, 0);
            }
        }
        // acc[g][s][r] = bf(v) . bf(x) of (item j0 + 16 s + 4 q + r, user q0 + 16 (UW wave + g) + ln)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const f32x4 h4 = *reinterpret_cast<const f32x4*>(th + cur * 64 + 16 * s + 4 * q);
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(tb + cur * 64 + 16 * s + 4 * q);
#pragma unroll
            for (int g = 0; g < UW; ++g) {
                if (thl[g] != thl[g]) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float tt = L2 ? __builtin_fmaf(2.0f, acc[g][s][r], h4[r]) : acc[g][s][r] + h4[r];
                    const float T = __builtin_fmaf(cA[g], b4[r], tt);
                    if (!(T < thl[g])) {                 // rare: into the workgroup's pool (an LDS atomic, no global round trip)
                        const int64_t j = j0 + 16 * s + 4 * q + r;
                        if (j < a.NI) {
                            const int slot = atomicAdd(pend, 1);
                            if (slot < a.pool_cap) a.pool_iu[pbase + slot] = make_int2((int)j, 16 * (UW * wave + g) + ln);
                        }
                    }
                }
            }
        }
        if (more) put(cur ^ 1);
        // a pool half full is emptied: one thread decides before the tile's barrier (it may miss this tile's last additions, the
        // next tile sees them), everybody reads the decision behind it -- no barrier of its own
        if (tid == 0) full[cur] = *reinterpret_cast<volatile int*>(pend) > a.pool_cap / 2;
        __syncthreads();
        if (full[cur]) flush();
    }
    flush();
}

// -------------------------------------------------------------------------------------------- rescore ---
// One workgroup per user, 256 candidates a round: wavefront w takes four MFMA tiles of 16 entries.  Tile row i holds the item of
// entry i, every column the user's row, and entry i's score is the diagonal element [i][i] (cand_score_kernel's construction: the
// scorer's operand layout and k order, all Dp columns, so the scorer's bits).  Survivors of s >= theta are written back to the front
// of the same list: a round writes only positions below the entries already read, behind the round's barrier.
__global__ __launch_bounds__(256) void topk16_rescore_kernel(Topk16RescoreArgs a) {
    extern __shared__ __attribute__((aligned(16))) float t16_user[];         // [Dp] the user operand row
    __shared__ int wcnt[2][4];
    __shared__ float s_un;
    const int64_t qu = blockIdx.x;
    const int n = a.cnt[qu];
    if (n > a.C || n <= 0) return;
    const int u = a.uid[qu];
    if ((uint32_t)u >= (uint64_t)a.NU) { *a.err = 1; return; }
    const int D = a.D, Dp = 16 * a.KB, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ii = lane & 15, kq = lane >> 4;
    const bool vec = (D & 3) == 0;
    for (int c = tid; c < Dp; c += 256) {
        float v = 0.0f;
        if (c < D) { v = a.U[(size_t)u * D + c]; if (a.kind == 2) v *= a.w[c]; }
        t16_user[c] = v;
    }
    __syncthreads();
    if (a.kind == 1 && tid == 0) {
        float s = 0.f;
        for (int c = 0; c < Dp; ++c) { const float x = t16_user[c]; s = __builtin_fmaf(x, x, s); }
        s_un = s;
    }
    if (tid == 0) atomicAdd(a.total, (unsigned long long)n);
    __syncthreads();
    const float un = a.kind == 1 ? s_un : 0.f;
    const float theta = a.theta[qu];
    const bool diag = kq == (ii >> 2);                     // this lane holds element [ii][ii] of a tile in acc[ii & 3]
    float* cs = a.cs + (size_t)qu * a.C;
    int32_t* ci = a.ci + (size_t)qu * a.C;
    int out = 0, round = 0;
    for (int base = 0; base < n; base += 256, ++round) {
        int item[4];
        f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int e = base + 64 * wave + 16 * t + ii;
            item[t] = e < n ? ci[e] : -1;
            if (item[t] >= a.NI) item[t] = -1;             // (never: the filter writes ids below NI)
            acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        for (int kb = 0; kb < a.KB; ++kb) {
            const int col = 16 * kb + 4 * kq;
            const f32x4 uf = *reinterpret_cast<const f32x4*>(t16_user + col);
            f32x4 cur[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                f32x4 z = {0.f, 0.f, 0.f, 0.f};
                if (item[t] >= 0) {
                    const float* row = a.V + (size_t)item[t] * D;
                    if (vec) { if (col < D) z = *reinterpret_cast<const f32x4*>(row + col); }
                    else {
#pragma unroll
                        for (int c = 0; c < 4; ++c) if (col + c < D) z[c] = row[col + c];
                    }
                }
                cur[t] = z;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[t][c], uf[c], acc[t], 0, 0, 0);
        }
        float sc[4];
        int rank[4];
        bool keep[4];
        int mine = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            keep[t] = false; sc[t] = 0.f;
            if (diag && item[t] >= 0) {
                const int r = ii & 3;
                float x = r == 0 ? acc[t][0] : (r == 1 ? acc[t][1] : (r == 2 ? acc[t][2] : acc[t][3]));
                if (a.kind == 1) x = 2.0f * x - un - a.nrm[item[t]];        // the scorer's element path
                sc[t] = a.b ? x + a.b[item[t]] : x;
                keep[t] = sc[t] >= theta;                                    // topk_filter_kernel's test: NaN is never a candidate
            }
            const unsigned long long bal = __ballot(keep[t]);
            rank[t] = mine + __popcll(bal & ((1ull << lane) - 1ull));
            mine += __popcll(bal);
        }
        if (lane == 0) wcnt[round & 1][wave] = mine;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w2 = 0; w2 < 4; ++w2) { const int c = wcnt[round & 1][w2]; all += c; if (w2 < wave) before += c; }
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (keep[t]) { const int pos = out + before + rank[t]; cs[pos] = sc[t]; ci[pos] = item[t]; }
        out += all;
    }
    if (tid == 0) a.cnt[qu] = out;
}

}  // namespace

// --------------------------------------------------------------------------------------------- launchers ---
int orx_launch_topk16_items(orx_ctx* ctx, const Topk16ItemArgs& a) {
    ProfScope ps(ctx, ORX_K_GEMM);
    const size_t lds = (size_t)T16_IR * (a.D + 1) * sizeof(float);
    ORX_LAUNCH(ctx, topk16_items_kernel, dim3((unsigned)(a.NIp / T16_IR)), dim3(256), lds, a);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

// the filter's shapes: users per workgroup 64 UW and k-blocks KBMAX, from the operand registers (4 UW nkb) and the user count
void orx_topk16_tile(int64_t nq, int D, int* UW, int* KBMAX) {
    const int nkb = (D + 31) / 32;
    *KBMAX = nkb <= 2 ? 2 : (nkb <= 4 ? 4 : 8);
    *UW = nq <= 64 ? 1 : (nq <= 128 || *KBMAX == 8 ? 2 : 4);
}

int64_t orx_topk16_chunk(int64_t nq, int64_t NIp, int UW) {
    const int64_t nqt = (nq + 64 * UW - 1) / (64 * UW);
    int64_t chunk = ((NIp * nqt + 1023) / 1024 + 63) / 64 * 64;
    if (chunk < 256) chunk = 256;
    if (chunk > 8192) chunk = 8192;
    const int64_t gx_max = TOPK_FILTER_BLOCKS / nqt;       // (the pools are sized for TOPK_FILTER_BLOCKS workgroups)
    if ((NIp + chunk - 1) / chunk > gx_max) chunk = ((NIp + gx_max - 1) / gx_max + 63) / 64 * 64;
    return chunk;
}

int orx_launch_topk16_filter(orx_ctx* ctx, Topk16FilterArgs a, bool l2) {
    int UW, KBMAX;
    orx_topk16_tile(a.nq, a.D, &UW, &KBMAX);
    const int64_t nqt = (a.nq + 64 * UW - 1) / (64 * UW);
    ORX_ARG(nqt <= TOPK_FILTER_BLOCKS, "topk16 filter: %lld user groups", (long long)nqt);
    a.chunk = orx_topk16_chunk(a.nq, a.NIp, UW);
    a.cmul = 1.05f * 0x1p-7f + (float)a.Dk * 0x1p-20f;
    a.err = ctx->d_err;
    const size_t lds = (size_t)2 * 64 * (2 * a.Dk + 16) + 256 * sizeof(float) + (3 + 2 * 64 * UW) * sizeof(int);
    const dim3 g((unsigned)((a.NIp + a.chunk - 1) / a.chunk), (unsigned)nqt);
    // the pools' memory is sized for TOPK_FILTER_BLOCKS workgroups: a launch of fewer gives each a larger share (a short item table
    // with a large k keeps a tenth of a tile's scores)
    a.pool_cap = (int)std::min<int64_t>(1 << 20, (int64_t)TOPK_FILTER_BLOCKS * TOPK_POOL / ((int64_t)g.x * g.y));
    ProfScope ps(ctx, ORX_K_GEMM);
#define ORX_T16(L, W, B) do { \
        ORX_ONCE_PER_DEVICE(ctx, ORX_HIP(hipFuncSetAttribute((const void*)topk16_filter_kernel<L, W, B>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024))); \
        ORX_LAUNCH(ctx, (topk16_filter_kernel<L, W, B>), g, dim3(256), lds, a); } while (0)
#define ORX_T16W(L, B) do { if (UW == 4) ORX_T16(L, 4, B); else if (UW == 2) ORX_T16(L, 2, B); else ORX_T16(L, 1, B); } while (0)
#define ORX_T16K(L) do { if (KBMAX == 2) ORX_T16W(L, 2); else if (KBMAX == 4) ORX_T16W(L, 4); \
                         else if (UW == 2) ORX_T16(L, 2, 8); else ORX_T16(L, 1, 8); } while (0)
    if (l2) ORX_T16K(true); else ORX_T16K(false);
#undef ORX_T16K
#undef ORX_T16W
#undef ORX_T16
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

int orx_launch_topk16_rescore(orx_ctx* ctx, Topk16RescoreArgs a, int64_t nq) {
    if (nq == 0) return ORX_OK;
    a.KB = 1;
    while (16 * a.KB < a.D) a.KB *= 2;
    a.err = ctx->d_err;
    ProfScope ps(ctx, ORX_K_GEMM);
    ORX_LAUNCH(ctx, topk16_rescore_kernel, dim3((unsigned)nq), dim3(256), (size_t)16 * a.KB * sizeof(float), a);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}
