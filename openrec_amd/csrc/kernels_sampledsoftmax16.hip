// The sampled softmax over a shared candidate list with bf16 operands on the matrix cores (ORX_SS_BF16; include/openrec_hip.h has
// the rounded semantics, DESIGN 4.5zb.1 the construction).  Where kernels_sampledsoftmax.hip gives a workgroup its 64 query rows
// across ALL of S -- B / 64 workgroups, a quarter of the machine at B = 4096 --, the row side here is split over row blocks x
// CANDIDATE CHUNKS, the twin of the column kernel's split over sample chunks, and the fused row kernel becomes three walks and two
// element-wise passes.  All three products run on v_mfma_f32_16x16x32_bf16; every sum stays fp32 (the accumulators, the online
// maximum, the Kahan running sums, the bias gradient), and no kernel before the applies writes a table.
//
//   ss16_gather_kernel  ss_gather_kernel with a second set of outputs: beside the fp32 xq / xp [Bp][Dp] and the per-row words it
//                       writes xq16 [Bp][Dk] and xc16 [Sp][Dk], the rows rounded to nearest even to bf16 (v_cvt_pk_bf16_f32, a lane
//                       takes two neighbouring columns), Dk = D rounded up to 32 -- one k-block of the instruction --, zeros beyond
//                       D, B and S.  s_i+ is formed here, from the rounded rows in fp32 (a product of two bf16 values is exact in
//                       fp32), so the label rows need no bf16 copy; the candidates need no fp32 copy (nothing regularises them).
//   ss16_stats_kernel   grid (Bp / 64, ncc).  A workgroup owns 64 query rows, wavefront w 16 of them, and walks the tpc candidate
//                       tiles of its chunk: the online (m, E) per lane, one Kahan term per tile; the four lane groups of a row
//                       merge in lane-group order into pm, pE [ncc][Bp].
//   ss16_merge_kernel   one thread per row: the chunks in chunk order, then the label's term exactly as ss_row_kernel joins it
//                       between its walks.  rmax, cn, rowloss, apos [Bp] and one (loss, l2) partial per 64 rows.
//   ss16_qgrad_kernel   grid (Bp / 64, ncc), only when the query side trains: S of the chunk again, turned into a_ic in the
//                       accumulator registers, G[own 16][Dp] += bf(a) . bf(X) into gqc [ncc][Bp][Dp].
//   ss16_col_kernel     grid (Sp / 64, ncs): ss_col_kernel's role on its sample-chunk plan.  64 candidate columns are the own rows,
//                       the query tiles of the chunk are walked out of xq16, a from the stored rmax / cn, G_c += bf(a)^T . bf(Q)
//                       into gpc, the Kahan sum of the UNROUNDED coefficients into bpc.
//   ss16_finish_kernel  one thread per element: gqc in chunk order, the label term and the l2 term into gu; the label entries
//                       into rows [0, B) of gi; gpc / bpc in chunk order into rows [B, B + S) of gi.
// The data path of a walk (stats, qgrad, col):
//   own rows      never touch LDS: lane (ln, q), lane = 16 q + ln, keeps k = 8 q .. 8 q + 7 of every k-block of own row ln in
//                 registers for the whole walk -- the B operand of the score product --, one 16-byte global load per k-block.
//   walked tile   16-byte global loads of tile t + 1 are in flight in registers under tile t; put() writes them row-major (pitch
//                 2 Dk + 16 bytes: an A operand is one ds_read_b128 per 16-row block and k-block, the 16 lanes of a lane group
//                 start 4 banks apart) and, in the two gradient walks, a second time transposed ([Dk][64 + 4] bf16).
//   S             four v_mfma_f32_16x16x32_bf16 per k-block into four interleaved accumulators; lane (ln, q) ends up with
//                 S[walked 16 s + 4 q + r][own ln] in acc[s][r].
//   G += a . X    the coefficients are rounded to bf16 where they sit and are the A operand (row = own ln): acc[0] | acc[1] fill the
//                 eight k-slots of one instruction, acc[2] | acc[3] those of a second, so k-slot j of lane group q in instruction h
//                 is walked row 16 (2 h + j / 4) + 4 q + j % 4.  The B operand presents X in the same k permutation,
//                 X[that row][16 gb + ln]: two ds_read_b64 of the transposed copy.  Two instructions per 16 columns and tile; lane
//                 (ln, q) ends up with G[own 4 q + r][16 gb + ln].
// Masking is a compare of keys, as in the fp32 kernels: a column whose key is < 0 is in nobody's softmax; with mask, neither is a
// column whose key is the row's own label.  A dead row has c = 0 and m = +inf.  No atomics: every sum has a fixed order that
// (B, S, D) alone determine, and the results are bit-repeatable.
#include <algorithm>

#include "orx_device.h"
#include "orx_mfma16.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr float SS_NEG = -3.0e38f;            // "no column yet": finite, so that exp(m - m) of an empty share is 1, not NaN
constexpr int SS16_TP = 64 + 4;               // the transposed copy's pitch in bf16: rows stay 8-byte aligned for ds_read_b64

// kernels_sampledsoftmax.hip ss_exp / ss_add, restated: v_exp_f32 of x log2(e) with the product's rounding error and the
// constant's low part put back to first order (below -104, and for the -inf of a masked column, 0); a Kahan running sum
__device__ __forceinline__ float ss_exp(float x) {
    x = fmaxf(x, -104.0f);
    const float hi = 1.44269502162933349609375f, lo = 1.92596299e-8f;
    const float t = x * hi;
    const float r = fmaf(x, lo, fmaf(x, hi, -t));
    const float e = __builtin_amdgcn_exp2f(t);
    return fmaf(e, r * 0.693147182f, e);
}

__device__ __forceinline__ void ss_add(float& s, float& c, float x) {
    const float y = x - c, t = s + y;
    c = (t - s) - y;
    s = t;
}

// x rounded to nearest even to bf16, as fp32
__device__ __forceinline__ float ss16_bf(float x) { return (float)(__bf16)x; }

// two fp32 -> two bf16, round to nearest even, as one word
__device__ __forceinline__ unsigned ss16_pack2(float lo, float hi) {
    bf16x2 v;
    v[0] = (__bf16)lo; v[1] = (__bf16)hi;
    return __builtin_bit_cast(unsigned, v);
}

// one wavefront per row, a lane two neighbouring columns at a time (Dp and Dk are even: a pair lies wholly inside a copy's row or
// wholly beyond it): the Bp query / label rows, then the Sp candidate rows
__global__ __launch_bounds__(256) void ss16_gather_kernel(SampledSoftmaxArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t < a.Bp) {
        const bool live = t < a.B;
        const int u = live ? a.qid[t] : 0, p = live ? a.pid[t] : 0;
        const bool ok = live && id_ok(u, a.NQ) && id_ok(p, a.NI);
        if (live && !ok && lane == 0) *a.err = 1;
        const float* qr = a.Q + (size_t)(ok ? u : 0) * a.D;
        const float* vr = a.V + (size_t)(ok ? p : 0) * a.D;
        float sq = 0.0f, dp = 0.0f;
        for (int c = 2 * lane; c < a.Dk; c += 128) {
            const bool in0 = ok && c < a.D, in1 = ok && c + 1 < a.D;
            const float x0 = in0 ? qr[c] : 0.0f, x1 = in1 ? qr[c + 1] : 0.0f;
            const float y0 = in0 ? vr[c] : 0.0f, y1 = in1 ? vr[c + 1] : 0.0f;
            if (c < a.Dp) {
                *reinterpret_cast<f32x2*>(a.xq + (size_t)t * a.Dp + c) = f32x2{x0, x1};
                *reinterpret_cast<f32x2*>(a.xp + (size_t)t * a.Dp + c) = f32x2{y0, y1};
            }
            *reinterpret_cast<unsigned*>(a.xq16 + (size_t)t * a.Dk + c) = ss16_pack2(x0, x1);
            sq = fmaf(x0, x0, fmaf(y0, y0, sq));
            sq = fmaf(x1, x1, fmaf(y1, y1, sq));
            dp = fmaf(ss16_bf(x0), ss16_bf(y0), dp);        // (the label's score: the rounded rows, an fp32 sum)
            dp = fmaf(ss16_bf(x1), ss16_bf(y1), dp);
        }
        sq = wave_sum(sq);
        dp = wave_sum(dp);
        if (lane == 0) {
            const float pb = (ok && a.b) ? a.b[p] : 0.0f, po = (ok && a.poff) ? a.poff[t] : 0.0f;
            a.key[t] = ok ? p : -1;
            a.pb[t] = pb;
            a.po[t] = po;
            a.spos[t] = fmaf(a.scale, dp + pb, po);         // s_i+
            a.cw[t] = ok ? (a.wt ? a.wt[t] : 1.0f) * a.invB : 0.0f;
            a.sq[t] = sq;
            if (a.list && live) a.list[t] = ok ? p : -1;
        }
        return;
    }
    const int64_t c = t - a.Bp;
    if (c >= a.Sp) return;
    const bool live = c < a.S;
    const int id = live ? a.cand[c] : 0;
    const bool ok = live && id_ok(id, a.NI);
    if (live && !ok && lane == 0) *a.err = 1;
    const float off = (ok && a.coff) ? a.coff[c] : 0.0f;
    const bool in = ok && off != -INFINITY;
    const float* vr = a.V + (size_t)(in ? id : 0) * a.D;
    for (int d = 2 * lane; d < a.Dk; d += 128) {
        const float x0 = (in && d < a.D) ? vr[d] : 0.0f, x1 = (in && d + 1 < a.D) ? vr[d + 1] : 0.0f;
        *reinterpret_cast<unsigned*>(a.xc16 + (size_t)c * a.Dk + d) = ss16_pack2(x0, x1);
    }
    if (lane == 0) {
        a.ckey[c] = in ? id : -1;
        a.cb[c] = (in && a.b) ? a.b[id] : 0.0f;
        a.co[c] = in ? off : 0.0f;
        if (a.list && live) a.list[a.B + c] = in ? id : -1;
    }
}

// LDS of a walk in bytes: the row-major tile, [the transposed tile], three words per walked row
__host__ __device__ inline size_t ss16_lds_bytes(int Dk, bool transposed) {
    return (size_t)64 * (2 * Dk + 16) + (transposed ? (size_t)Dk * SS16_TP * 2 : 0) + 192 * sizeof(float);
}

// One walk.  MODE 0: the stats of a candidate chunk; 1: the query gradient of a candidate chunk; 2: the candidates' gradient of a
// sample chunk.  MODE 0 / 1 own query rows and walk candidate tiles (their keys, biases, offsets); MODE 2 owns candidate columns
// and walks query tiles (their label keys, c / tot, maxima).  KBMAX: the power of two at or above Dk / 32
template <int MODE, int KBMAX>
__device__ __forceinline__ void ss16_walk(const SampledSoftmaxArgs& a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ss16_lds[];
    const int Dk = a.Dk, nkb = Dk >> 5, ngb = a.Dp >> 4, pitch = 2 * Dk + 16, c8n = Dk >> 3;
    unsigned char* Bs = ss16_lds;                                        // [64][pitch bytes] the tile of walked rows, row-major
    unsigned short* Bt = reinterpret_cast<unsigned short*>(Bs + 64 * pitch);        // [Dk][SS16_TP] the same tile transposed (MODE 1 / 2)
    int* wkey = reinterpret_cast<int*>(Bt + (MODE == 0 ? 0 : Dk * SS16_TP));        // [64] the tile's keys
    float* wa = reinterpret_cast<float*>(wkey + 64);        // [64] MODE 0 / 1: the tile's biases;  MODE 2: its c / tot
    float* wb = wa + 64;                                    // [64] MODE 0 / 1: the tile's offsets; MODE 2: its row maxima
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, ln = lane & 15;
    const unsigned short* Xo = MODE == 2 ? a.xc16 : a.xq16;
    const unsigned short* Xw = MODE == 2 ? a.xq16 : a.xc16;
    const int32_t* kw = MODE == 2 ? a.key : a.ckey;
    const float* fa = MODE == 2 ? a.cn : a.cb;
    const float* fb = MODE == 2 ? a.rmax : a.co;
    const int64_t no = MODE == 2 ? a.Sp : a.Bp;             // own rows in all: the pitch of a chunk's partials
    const int64_t o0 = (int64_t)blockIdx.x * 64;
    const int chunk = blockIdx.y;
    const int ntiles = (int)((MODE == 2 ? a.Bp : a.Sp) >> 6), tpc = MODE == 2 ? a.tps : a.tpc;
    const int t_beg = chunk * tpc;
    const int t_end = t_beg + tpc < ntiles ? t_beg + tpc : ntiles;
    // this lane's own row: 16 per wavefront, the same one in the four lane groups
    const int64_t o = o0 + 16 * wave + ln;
    bf16x8 ov[KBMAX];
#pragma unroll
    for (int kb = 0; kb < KBMAX; ++kb)
        ov[kb] = __builtin_bit_cast(bf16x8, kb < nkb ? *reinterpret_cast<const u32x4*>(Xo + (size_t)o * Dk + 32 * kb + 8 * q) : u32x4{0u, 0u, 0u, 0u});
    u32x4 stage[KBMAX];
    int skey = 0;
    float sa = 0.0f, sb = 0.0f;
    auto fetch = [&](int tile) {
        const u32x4* src = reinterpret_cast<const u32x4*>(Xw + (size_t)tile * 64 * Dk);     // 64 c8n = 256 nkb groups of eight, contiguous
#pragma unroll
        for (int k = 0; k < KBMAX; ++k)
            if (k < nkb) stage[k] = src[tid + 256 * k];
        if (tid < 64) {
            const int64_t t = (int64_t)tile * 64 + tid;
            skey = kw[t]; sa = fa[t]; sb = fb[t];
        }
    };
    auto put = [&]() {
#pragma unroll
        for (int k = 0; k < KBMAX; ++k)
            if (k < nkb) {
                const int e = tid + 256 * k, r = e / c8n, c = e - r * c8n;
                *reinterpret_cast<u32x4*>(Bs + r * pitch + 16 * c) = stage[k];
                if (MODE != 0) {
                    unsigned short* col = Bt + (8 * c) * SS16_TP + r;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        col[(2 * j) * SS16_TP] = (unsigned short)(stage[k][j] & 0xffffu);
                        col[(2 * j + 1) * SS16_TP] = (unsigned short)(stage[k][j] >> 16);
                    }
                }
            }
        if (tid < 64) { wkey[tid] = skey; wa[tid] = sa; wb[tid] = sb; }
    };
    const int okey = MODE == 2 ? a.ckey[o] : a.key[o];
    const float own_a = MODE == 1 ? a.cn[o] : (MODE == 2 ? a.cb[o] : 0.0f);       // query side: c_i / tot_i; candidate side: b_c
    const float own_b = MODE == 1 ? a.rmax[o] : (MODE == 2 ? a.co[o] : 0.0f);     // query side: m_i;         candidate side: off_c
    const float scale = a.scale;
    const bool mask = a.mask != 0;
    float m = SS_NEG, E = 0.0f, Ec = 0.0f;                  // MODE 0
    float bsum = 0.0f, bc = 0.0f;                           // MODE 2
    constexpr int GB = MODE == 0 ? 1 : 2 * KBMAX;           // 16-column blocks of G
    f32x4 G[GB];
#pragma unroll
    for (int k = 0; k < GB; ++k) G[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    const unsigned char* wrow = Bs + ln * pitch + 16 * q;
    const unsigned short* xcol = Bt + ln * SS16_TP + 4 * q;

    fetch(t_beg);
    put();
    __syncthreads();
    for (int tile = t_beg; tile < t_end; ++tile) {
        const bool more = tile + 1 < t_end;
        if (more) fetch(tile + 1);
        f32x4 acc[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < KBMAX; ++kb) {
            if (kb < nkb) {
                bf16x8 wv[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) wv[s] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(wrow + s * 16 * pitch + 64 * kb));
                // four independent accumulators, interleaved: consecutive MFMAs never wait for each other's result
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv[s], ov[kb], acc[s], 0, 0, 0);
            }
        }
        // acc[s][r] = bf(x) . bf(y) of (walked row 64 tile + 16 s + 4 q + r, own row o)
        float tmax = SS_NEG, tsum = 0.0f;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int base = 16 * s + 4 * q;
            const i32x4 k4 = *reinterpret_cast<const i32x4*>(wkey + base);
            const f32x4 a4 = *reinterpret_cast<const f32x4*>(wa + base);
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(wb + base);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool out = k4[r] < 0 || okey < 0 || (mask && k4[r] == okey);
                if (MODE == 0) {
                    acc[s][r] = out ? -INFINITY : fmaf(scale, acc[s][r] + a4[r], b4[r]);
                    tmax = fmaxf(tmax, acc[s][r]);
                } else if (MODE == 1) {
                    const float sc = fmaf(scale, acc[s][r] + a4[r], b4[r]);
                    acc[s][r] = out ? 0.0f : own_a * ss_exp(sc - own_b);          // a_ic, where it sits
                } else {
                    const float sc = fmaf(scale, acc[s][r] + own_a, own_b);
                    const float co = out ? 0.0f : a4[r] * ss_exp(sc - b4[r]);
                    acc[s][r] = co;
                    tsum += co;
                }
            }
        }
        if (MODE == 0) {
            const float mn = fmaxf(m, tmax);
            float e = 0.0f;
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r) e += ss_exp(acc[s][r] - mn);
            const float f = ss_exp(m - mn);
            E *= f; Ec *= f;
            ss_add(E, Ec, e);
            m = mn;
        } else {
            if (MODE == 2) ss_add(bsum, bc, tsum);          // (the unrounded coefficients)
            bf16x8 co[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) co[h] = __builtin_bit_cast(bf16x8, fs16_pack(acc[2 * h], acc[2 * h + 1]));
#pragma unroll
            for (int gb = 0; gb < GB; ++gb)
                if (gb < ngb) {
                    const unsigned short* xc = xcol + 16 * gb * SS16_TP;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const u32x2 x0 = *reinterpret_cast<const u32x2*>(xc + 32 * h), x1 = *reinterpret_cast<const u32x2*>(xc + 32 * h + 16);
                        const u32x4 x = u32x4{x0[0], x0[1], x1[0], x1[1]};
                        G[gb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(co[h], __builtin_bit_cast(bf16x8, x), G[gb], 0, 0, 0);
                    }
                }
        }
        __syncthreads();                      // every wavefront is done with the tile
        if (more) put();
        __syncthreads();
    }
    const size_t prow = (size_t)chunk * no;
    if (MODE == 0) {
        // the four lane groups of a row, in lane-group order
        float M = SS_NEG, mk[4], Ek[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            mk[k] = __shfl(m, ln + 16 * k); Ek[k] = __shfl(E, ln + 16 * k);
            M = fmaxf(M, mk[k]);
        }
        float Es = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) Es = fmaf(Ek[k], ss_exp(mk[k] - M), Es);
        if (q == 0) { a.pm[prow + o] = M; a.pE[prow + o] = Es; }
    } else {
        // G[gb][r] is (own row 16 wave + 4 q + r, column 16 gb + ln) of this chunk's partial tile
        float* gp = (MODE == 2 ? a.gpc : a.gqc) + (prow + (size_t)o0 + 16 * wave + 4 * q) * a.Dp + ln;
#pragma unroll
        for (int gb = 0; gb < GB; ++gb)
            if (gb < ngb) {
#pragma unroll
                for (int r = 0; r < 4; ++r) gp[(size_t)r * a.Dp + 16 * gb] = G[gb][r];
            }
        if (MODE == 2) {
            bsum += __shfl_xor(bsum, 16);
            bsum += __shfl_xor(bsum, 32);
            if (q == 0) a.bpc[prow + o] = bsum;
        }
    }
}

template <int KBMAX>
__global__ __launch_bounds__(256) void ss16_stats_kernel(SampledSoftmaxArgs a) { ss16_walk<0, KBMAX>(a); }
template <int KBMAX>
__global__ __launch_bounds__(256) void ss16_qgrad_kernel(SampledSoftmaxArgs a) { ss16_walk<1, KBMAX>(a); }
template <int KBMAX>
__global__ __launch_bounds__(256) void ss16_col_kernel(SampledSoftmaxArgs a) { ss16_walk<2, KBMAX>(a); }

// one thread per row, a wavefront per 64 rows: the candidate chunks in chunk order, then the label's own term
__global__ __launch_bounds__(64) void ss16_merge_kernel(SampledSoftmaxArgs a) {
    const int64_t o = (int64_t)blockIdx.x * 64 + threadIdx.x;
    float M = SS_NEG;
    for (int ch = 0; ch < a.ncc; ++ch) M = fmaxf(M, a.pm[(size_t)ch * a.Bp + o]);
    float Es = 0.0f;
    for (int ch = 0; ch < a.ncc; ++ch) Es = fmaf(a.pE[(size_t)ch * a.Bp + o], ss_exp(a.pm[(size_t)ch * a.Bp + o] - M), Es);
    const float sp = a.spos[o], cw = a.cw[o];
    float l = 0.0f, rmax = INFINITY, cn = 0.0f, apos = 0.0f;
    if (a.key[o] >= 0) {
        const float M2 = fmaxf(M, sp);
        const float Eo = Es * ss_exp(M - M2);                  // the candidates' sum at the row maximum
        const float tot = ss_exp(sp - M2) + Eo;                // (the label's term is exactly 1 when it holds the maximum)
        l = sp == M2 ? log1pf(Eo) : (M2 - sp) + logf(tot);
        rmax = M2;
        cn = cw / tot;
        apos = -cn * Eo;                                       // -c_i sum_c pi_ic: the pi themselves, never 1 - pi_+
    }
    a.rmax[o] = rmax; a.cn[o] = cn; a.rowloss[o] = l; a.apos[o] = apos;
    const float cl = wave_sum(cw * l), sq = wave_sum(a.sq[o]);
    if (threadIdx.x == 0) {
        float2 v;
        v.x = cl;
        v.y = 0.5f * sq;
        *reinterpret_cast<float2*>(a.partial + 2 * (size_t)blockIdx.x) = v;
    }
}

// one thread per element of a gradient row: [gu: B gs query elements] [gi: B gs label elements, S gs candidate elements]
__global__ __launch_bounds__(256) void ss16_finish_kernel(SampledSoftmaxArgs a) {
    int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t nb = a.B * a.gs;
    const int D = a.D, gs = a.gs;
    if (a.gu) {
        if (idx < nb) {
            const int64_t i = idx / gs;
            const int d = (int)(idx - i * gs);
            float g = 0.0f;
            if (d < D) {
                for (int ch = 0; ch < a.ncc; ++ch) g += a.gqc[((size_t)ch * a.Bp + i) * a.Dp + d];
                g = fmaf(a.scale, fmaf(a.apos[i], ss16_bf(a.xp[(size_t)i * a.Dp + d]), g), a.l2w * a.xq[(size_t)i * a.Dp + d]);
            }
            a.gu[idx] = g;
            return;
        }
        idx -= nb;
    }
    if (!a.gi) return;
    if (idx < nb) {                             // the label entry of sample i, the bias gradient in column D
        const int64_t i = idx / gs;
        const int d = (int)(idx - i * gs);
        float g = 0.0f;
        if (d < D) g = fmaf(a.scale * a.apos[i], ss16_bf(a.xq[(size_t)i * a.Dp + d]), a.l2w * a.xp[(size_t)i * a.Dp + d]);
        else if (d == D) g = a.scale * a.apos[i];
        a.gi[idx] = g;
        return;
    }
    idx -= nb;
    if (idx >= a.S * gs) return;
    const int64_t c = idx / gs;                 // candidate c: the sample chunks in chunk order, the scale; no l2 on a candidate
    const int d = (int)(idx - c * gs);
    float g = 0.0f;
    if (d < D) {
        for (int ch = 0; ch < a.ncs; ++ch) g += a.gpc[((size_t)ch * a.Sp + c) * a.Dp + d];
        g *= a.scale;
    } else if (d == D) {
        for (int ch = 0; ch < a.ncs; ++ch) g += a.bpc[(size_t)ch * a.Sp + c];
        g *= a.scale;
    }
    a.gi[nb + idx] = g;
}

// MODE as in ss16_walk; the two gradient walks at D = 256 need 68 KB of LDS, above the 64 KB a kernel gets unasked
template <int MODE>
int ss16_launch_walk(orx_ctx* ctx, const SampledSoftmaxArgs& a) {
    const dim3 g((unsigned)((MODE == 2 ? a.Sp : a.Bp) >> 6), (unsigned)(MODE == 2 ? a.ncs : a.ncc));
    const size_t lds = ss16_lds_bytes(a.Dk, MODE != 0);
    int kbmax = 1;
    while (32 * kbmax < a.Dk) kbmax *= 2;
#define ORX_SS16(KERNEL, KB) do { \
        ORX_ONCE_PER_DEVICE(ctx, ORX_HIP(hipFuncSetAttribute((const void*)KERNEL<KB>, hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024))); \
        ORX_LAUNCH(ctx, (KERNEL<KB>), g, dim3(256), lds, a); } while (0)
#define ORX_SS16_KB(KB) do { \
        if (MODE == 0) ORX_SS16(ss16_stats_kernel, KB); else if (MODE == 1) ORX_SS16(ss16_qgrad_kernel, KB); else ORX_SS16(ss16_col_kernel, KB); } while (0)
    switch (kbmax) {
        case 1: ORX_SS16_KB(1); break;
        case 2: ORX_SS16_KB(2); break;
        case 4: ORX_SS16_KB(4); break;
        default: ORX_SS16_KB(8); break;
    }
#undef ORX_SS16_KB
#undef ORX_SS16
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

}  // namespace

// the fp32 plan's padded sizes and sample chunks, and the candidate chunks of the row side -- the twin of the column plan: it aims
// at 512 workgroups and keeps at least four tiles per chunk; a function of (B, S) alone
void orx_sampledsoftmax16_plan(int64_t B, int64_t S, int32_t D, SampledSoftmaxPlan* p) {
    orx_sampledsoftmax_plan(B, S, D, p);
    p->Dk = (D + 31) & ~31;
    const int64_t ntiles = p->Sp >> 6;
    const int64_t want = std::max<int64_t>(1, 512 / std::max<int64_t>(1, p->Bp >> 6));
    p->tpc = std::min<int64_t>(ntiles, std::max<int64_t>(4, (ntiles + want - 1) / want));
    p->ncc = (ntiles + p->tpc - 1) / p->tpc;
}

int orx_launch_sampledsoftmax16_forward(orx_ctx* ctx, const SampledSoftmaxArgs& a) {
    {
        ProfScope ps(ctx, ORX_K_FUSED);
        ORX_LAUNCH(ctx, ss16_gather_kernel, dim3((unsigned)((a.Bp + a.Sp + 3) / 4)), dim3(256), 0, a);
        ORX_HIP(hipGetLastError());
    }
    {
        ProfScope ps(ctx, ORX_K_GEMM);
        CHECK(ss16_launch_walk<0>(ctx, a));
    }
    ProfScope ps(ctx, ORX_K_FUSED);
    ORX_LAUNCH(ctx, ss16_merge_kernel, dim3((unsigned)(a.Bp >> 6)), dim3(64), 0, a);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

int orx_launch_sampledsoftmax16_grads(orx_ctx* ctx, const SampledSoftmaxArgs& a) {
    if (!a.gu && !a.gi) return ORX_OK;
    if (a.gu) {                                 // (a profiling scope times one dispatch)
        ProfScope ps(ctx, ORX_K_GEMM);
        CHECK(ss16_launch_walk<1>(ctx, a));
    }
    if (a.gi && a.S) {
        ProfScope ps(ctx, ORX_K_GEMM);
        CHECK(ss16_launch_walk<2>(ctx, a));
    }
    ProfScope ps(ctx, ORX_K_FUSED);
    const int64_t n = (a.gu ? a.B * a.gs : 0) + (a.gi ? (a.B + a.S) * a.gs : 0);
    ORX_LAUNCH(ctx, ss16_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, a);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}
