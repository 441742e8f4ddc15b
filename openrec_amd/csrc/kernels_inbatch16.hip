// In-batch negatives with bf16 operands on the matrix cores (ORX_IB_BF16; include/openrec_hip.h has the rounded semantics, DESIGN
// 4.5n.1 the construction): the gather and the three walks of kernels_inbatch.hip restated around v_mfma_f32_16x16x32_bf16.
// Everything else is that file's: the partial buffers have its layout, and its finalize, finish and loss-reduce kernels run
// unchanged on the fp32 copies xu / xv.  Sums stay fp32: the accumulators, the online maximum, the Kahan running sums, the bias
// gradient.
//
//   inbatch16_gather_kernel  inbatch_gather_kernel with a second pair of outputs: beside xu / xv [Bp][Dp] and the per-sample words it
//                            writes xu16 / xv16 [Bp][Dk], the rows rounded to nearest even to bf16 (v_cvt_pk_bf16_f32, a lane takes two
//                            neighbouring columns), Dk = D rounded up to 32 -- one k-block of the instruction --, zeros beyond D and B.
//   inbatch16_walk_kernel<MODE>  the roles of inbatch_walk_kernel: a workgroup owns 64 rows (wavefront w 16 of them) and walks the
//                            64-row tiles of its chunk.  Data path:
//     own rows      never touch LDS: lane (ln, q) keeps k = 8 q .. 8 q + 7 of every k-block of own row ln in registers for the
//                   whole walk (the B operand of the first product), one 16-byte global load per k-block.
//     walked tile   16-byte global loads of tile t + 1 are in flight under tile t; put() writes them row-major (pitch 2 Dk + 16
//                   bytes: the A operand is one ds_read_b128 per 16-row block and k-block) and, in the gradient modes, a second
//                   time transposed ([Dk][64 + 4] bf16).
//     S             four v_mfma_f32_16x16x32_bf16 per k-block into four interleaved accumulators; lane (ln, q) ends up with
//                   S[walked 16 s + 4 q + r][own ln], the fp32 walk's layout.
//     epilogue      this objective's, statement for statement the fp32 walk's: the keys of the walked tile against the own row's
//                   (a dead row or column, a hit), the diagonal taking -c_i A_i, exp without a logarithm, one Kahan term per tile;
//                   on the item side m and c / tot are the walked rows' and b, off the own row's, and the sum of the UNROUNDED
//                   coefficients of an own row is the bias gradient.
//     G += a . X    the coefficients are rounded to bf16 where they sit and are the A operand: acc[0] | acc[1] fill the eight k-slots
//                   of one instruction, acc[2] | acc[3] those of a second.  The B operand presents X in the same k permutation,
//                   X[16 s + 4 q + r][16 gb + ln]: two ds_read_b64 of the transposed copy.  Two instructions per 16 columns and tile.
// No atomics: every sum has a fixed order, and the results are bit-repeatable.
#include "orx_device.h"
#include "orx_mfma16.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr float IB_NEG = -3.0e38f;            // "no column yet": finite, so that exp(m - m) of an empty share is 1, not NaN
constexpr int IB16_TP = 64 + 4;               // the transposed copy's pitch in bf16: rows stay 8-byte aligned for ds_read_b64

// kernels_inbatch.hip ib_exp / ib_add, restated: v_exp_f32 of x log2(e) with the product's rounding error and the constant's low
// part put back to first order; a Kahan-compensated running sum
__device__ __forceinline__ float ib_exp(float x) {
    x = fmaxf(x, -104.0f);
    const float hi = 1.44269502162933349609375f, lo = 1.92596299e-8f;
    const float t = x * hi;
    const float r = fmaf(x, lo, fmaf(x, hi, -t));
    const float e = __builtin_amdgcn_exp2f(t);
    return fmaf(e, r * 0.693147182f, e);
}

__device__ __forceinline__ void ib_add(float& s, float& c, float x) {
    const float y = x - c, t = s + y;
    c = (t - s) - y;
    s = t;
}

// two fp32 -> two bf16, round to nearest even, as one word
__device__ __forceinline__ unsigned ib16_pack2(float lo, float hi) {
    bf16x2 v;
    v[0] = (__bf16)lo; v[1] = (__bf16)hi;
    return __builtin_bit_cast(unsigned, v);
}

// eight fp32 -> eight bf16 as 16 bytes
__device__ __forceinline__ u32x4 ib16_pack8(f32x4 lo, f32x4 hi) {
    return u32x4{ib16_pack2(lo[0], lo[1]), ib16_pack2(lo[2], lo[3]), ib16_pack2(hi[0], hi[1]), ib16_pack2(hi[2], hi[3])};
}

// one wavefront per sample, a lane two neighbouring columns at a time (Dp and Dk are even: a pair lies wholly inside a copy's row
// or wholly beyond it)
__global__ __launch_bounds__(256) void inbatch16_gather_kernel(InBatchArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= a.Bp) return;
    const bool live = t < a.B;
    const int u = live ? a.uid[t] : 0, p = live ? a.pid[t] : 0;
    const bool ok = live && id_ok(u, a.NU) && id_ok(p, a.NI);
    if (live && !ok && lane == 0) *a.err = 1;
    const float* ur = a.U + (size_t)(ok ? u : 0) * a.D;
    const float* vr = a.V + (size_t)(ok ? p : 0) * a.D;
    float sq = 0.0f;
    for (int c = 2 * lane; c < a.Dk; c += 128) {
        const bool in0 = ok && c < a.D, in1 = ok && c + 1 < a.D;
        const float x0 = in0 ? ur[c] : 0.0f, x1 = in1 ? ur[c + 1] : 0.0f;
        const float y0 = in0 ? vr[c] : 0.0f, y1 = in1 ? vr[c + 1] : 0.0f;
        if (c < a.Dp) {
            *reinterpret_cast<f32x2*>(a.xu + (size_t)t * a.Dp + c) = f32x2{x0, x1};
            *reinterpret_cast<f32x2*>(a.xv + (size_t)t * a.Dp + c) = f32x2{y0, y1};
        }
        *reinterpret_cast<unsigned*>(a.xu16 + (size_t)t * a.Dk + c) = ib16_pack2(x0, x1);
        *reinterpret_cast<unsigned*>(a.xv16 + (size_t)t * a.Dk + c) = ib16_pack2(y0, y1);
        sq = fmaf(x0, x0, fmaf(y0, y0, sq));
        sq = fmaf(x1, x1, fmaf(y1, y1, sq));
    }
    sq = wave_sum(sq);
    if (lane == 0) {
        a.key[t] = ok ? p : -1;
        a.cb[t] = (ok && a.b) ? a.b[p] : 0.0f;
        a.co[t] = (ok && a.off) ? a.off[t] : 0.0f;
        a.cw[t] = ok ? (a.wt ? a.wt[t] : 1.0f) * a.invB : 0.0f;
        a.sq[t] = sq;
    }
}

// MODE 0: the LSE pass; 1: the gradients of the user side; 2: of the item side.  KBMAX: the power of two at or above Dk / 32
template <int MODE, int KBMAX>
__global__ __launch_bounds__(256) void inbatch16_walk_kernel(InBatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ib16_lds[];
    const int Dk = a.Dk, nkb = Dk >> 5, ngb = a.Dp >> 4, pitch = 2 * Dk + 16, c8n = Dk >> 3;
    unsigned char* Bs = ib16_lds;                                        // [64][pitch bytes] the tile of walked rows, row-major
    unsigned short* Bt = reinterpret_cast<unsigned short*>(Bs + 64 * pitch);        // [Dk][IB16_TP] the same tile transposed (MODE 1 / 2)
    int* wkey = reinterpret_cast<int*>(Bt + (MODE == 0 ? 0 : Dk * IB16_TP));        // [64] the tile's keys
    float* wa = reinterpret_cast<float*>(wkey + 64);        // [64] MODE 0 / 1: the tile's biases;  MODE 2: its c / tot
    float* wb = wa + 64;                                    // [64] MODE 0 / 1: the tile's offsets; MODE 2: its row maxima
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, ln = lane & 15;
    const unsigned short* Xo = MODE == 2 ? a.xv16 : a.xu16;
    const unsigned short* Xw = MODE == 2 ? a.xu16 : a.xv16;
    const int64_t o0 = (int64_t)blockIdx.x * 64;
    const int chunk = blockIdx.y;
    const int ntiles = (int)(a.Bp >> 6);
    const int t_beg = chunk * a.tpc;
    const int t_end = t_beg + a.tpc < ntiles ? t_beg + a.tpc : ntiles;
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
            skey = a.key[t];
            sa = MODE == 2 ? a.cn[t] : a.cb[t];
            sb = MODE == 2 ? a.rmax[t] : a.co[t];
        }
    };
    auto put = [&]() {
#pragma unroll
        for (int k = 0; k < KBMAX; ++k)
            if (k < nkb) {
                const int e = tid + 256 * k, r = e / c8n, c = e - r * c8n;
                *reinterpret_cast<u32x4*>(Bs + r * pitch + 16 * c) = stage[k];
                if (MODE != 0) {
                    unsigned short* col = Bt + (8 * c) * IB16_TP + r;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        col[(2 * j) * IB16_TP] = (unsigned short)(stage[k][j] & 0xffffu);
                        col[(2 * j + 1) * IB16_TP] = (unsigned short)(stage[k][j] >> 16);
                    }
                }
            }
        if (tid < 64) { wkey[tid] = skey; wa[tid] = sa; wb[tid] = sb; }
    };
    const int okey = a.key[o];
    const float own_a = MODE == 1 ? a.cn[o] : (MODE == 2 ? a.cb[o] : 0.0f);       // user side: c_i / tot_i; item side: b_j
    const float own_b = MODE == 1 ? a.rmax[o] : (MODE == 2 ? a.co[o] : 0.0f);     // user side: m_i;         item side: off_j
    const float dco = MODE == 0 ? 0.0f : a.dcoef[o];        // the diagonal is row o of either side
    const float scale = a.scale;
    const bool mask = a.mask != 0;
    float m = IB_NEG, E = 0.0f, Ec = 0.0f, sd = -INFINITY;  // MODE 0
    float bsum = 0.0f, bc = 0.0f;                           // MODE 2
    constexpr int GB = MODE == 0 ? 1 : 2 * KBMAX;           // 16-column blocks of G
    f32x4 G[GB];
#pragma unroll
    for (int k = 0; k < GB; ++k) G[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    const unsigned char* wrow = Bs + ln * pitch + 16 * q;
    const unsigned short* xcol = Bt + ln * IB16_TP + 4 * q;

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
        // acc[s][r] = bf(u) . bf(v) of (walked row 64 tile + 16 s + 4 q + r, own row o)
        float tmax = IB_NEG, tsum = 0.0f;
        unsigned diagbits = 0;                              // which of this lane's 16 walked rows is its own row
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int base = 16 * s + 4 * q;
            const i32x4 k4 = *reinterpret_cast<const i32x4*>(wkey + base);
            const f32x4 a4 = *reinterpret_cast<const f32x4*>(wa + base);
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(wb + base);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t t = (int64_t)tile * 64 + base + r;
                const int kt = k4[r];
                const bool diag = t == o;
                const bool out = kt < 0 || okey < 0 || (mask && !diag && kt == okey);
                if (diag) diagbits |= 1u << (4 * s + r);
                if (MODE == 0) {
                    const float sc = out ? -INFINITY : fmaf(scale, acc[s][r] + a4[r], b4[r]);
                    if (diag) sd = sc;
                    acc[s][r] = sc;
                    tmax = fmaxf(tmax, sc);
                } else if (MODE == 1) {
                    const float sc = fmaf(scale, acc[s][r] + a4[r], b4[r]);
                    const float pi = out ? 0.0f : own_a * ib_exp(sc - own_b);
                    acc[s][r] = diag ? dco : pi;
                } else {
                    const float sc = fmaf(scale, acc[s][r] + own_a, own_b);
                    const float pi = out ? 0.0f : a4[r] * ib_exp(sc - b4[r]);
                    const float co = diag ? dco : pi;
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
                for (int r = 0; r < 4; ++r) e += ((diagbits >> (4 * s + r)) & 1u) ? 0.0f : ib_exp(acc[s][r] - mn);
            const float f = ib_exp(m - mn);
            E *= f; Ec *= f;
            ib_add(E, Ec, e);
            m = mn;
        } else {
            if (MODE == 2) ib_add(bsum, bc, tsum);          // (the unrounded coefficients)
            // G[own 16][Dp] += bf(a)[own 16][64 walked] . X[64 walked][Dp]: k-slot j of lane group q is walked row
            // 16 (2 h + j / 4) + 4 q + j % 4 in instruction h, for the coefficients as they sit and for the transposed tile alike
            bf16x8 co[2];
#pragma unroll
            for (int h = 0; h < 2; ++h)
                co[h] = __builtin_bit_cast(bf16x8, ib16_pack8(acc[2 * h], acc[2 * h + 1]));
#pragma unroll
            for (int gb = 0; gb < GB; ++gb)
                if (gb < ngb) {
                    const unsigned short* xc = xcol + 16 * gb * IB16_TP;
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
    const size_t prow = (size_t)chunk * a.Bp;
    if (MODE == 0) {
        // the four lane groups of a row, in lane-group order
        float M = IB_NEG, mk[4], Ek[4], sdm = -INFINITY;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            mk[k] = __shfl(m, ln + 16 * k); Ek[k] = __shfl(E, ln + 16 * k);
            sdm = fmaxf(sdm, __shfl(sd, ln + 16 * k));
            M = fmaxf(M, mk[k]);
        }
        float Es = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) Es = fmaf(Ek[k], ib_exp(mk[k] - M), Es);
        if (q == 0) { a.pm[prow + o] = M; a.pe[prow + o] = Es; a.psd[prow + o] = sdm; }
    } else {
        // the partial tiles have the fp32 walk's layout, [chunk][row][Dp]: inbatch_finish_kernel reads them
        float* gp = (MODE == 2 ? a.gpv : a.gpu) + (prow + (size_t)o0 + 16 * wave + 4 * q) * a.Dp + ln;
#pragma unroll
        for (int gb = 0; gb < GB; ++gb)
            if (gb < ngb) {
#pragma unroll
                for (int r = 0; r < 4; ++r) gp[(size_t)r * a.Dp + 16 * gb] = G[gb][r];
            }
        if (MODE == 2) {
            bsum += __shfl_xor(bsum, 16);
            bsum += __shfl_xor(bsum, 32);
            if (q == 0) a.bpart[prow + o] = bsum;
        }
    }
}

template <int MODE>
int ib16_walk(orx_ctx* ctx, const InBatchArgs& a) {
    const dim3 g((unsigned)(a.Bp >> 6), (unsigned)a.nch);
    const size_t lds = (size_t)64 * (2 * a.Dk + 16) + (MODE == 0 ? 0 : (size_t)a.Dk * IB16_TP * 2) + 192 * sizeof(float);
    int kbmax = 1;
    while (32 * kbmax < a.Dk) kbmax *= 2;
#define ORX_IB16(KB) do { \
        ORX_ONCE_PER_DEVICE(ctx, ORX_HIP(hipFuncSetAttribute((const void*)inbatch16_walk_kernel<MODE, KB>, hipFuncAttributeMaxDynamicSharedMemorySize, 112 * 1024))); \
        ORX_LAUNCH(ctx, (inbatch16_walk_kernel<MODE, KB>), g, dim3(256), lds, a); } while (0)
    switch (kbmax) {
        case 1: ORX_IB16(1); break;
        case 2: ORX_IB16(2); break;
        case 4: ORX_IB16(4); break;
        default: ORX_IB16(8); break;
    }
#undef ORX_IB16
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

}  // namespace

int orx_launch_inbatch16_gather(orx_ctx* ctx, const InBatchArgs& a) {
    ORX_LAUNCH(ctx, inbatch16_gather_kernel, dim3((unsigned)((a.Bp + 3) / 4)), dim3(256), 0, a);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

int orx_launch_inbatch16_walk(orx_ctx* ctx, const InBatchArgs& a, int mode) {
    return mode == 0 ? ib16_walk<0>(ctx, a) : mode == 1 ? ib16_walk<1>(ctx, a) : ib16_walk<2>(ctx, a);
}
