// The full softmax over all items with bf16 operands on the matrix cores (ORX_FS_BF16; include/openrec_hip.h has the rounded
// semantics, DESIGN 4.5w the construction): the three walks of kernels_fullsoftmax.hip restated around
// v_mfma_f32_16x16x32_bf16.  Everything but the walks is that file's: fs_prepare_kernel and fs_items_kernel still write the fp32
// copies xq / xv (the l2 terms of finalize and finish read them), the partial buffers have its layout, and its finalize and
// finish kernels run unchanged.  Sums stay fp32: the accumulators, the online maximum, the Kahan running sums, the bias gradient.
//
//   fs16_copy_kernel         xq16 [Bp][Dk] and xv16 [NIp][Dk], the bf16 (round-to-nearest-even) copies of xq and xv; Dk = D rounded
//                            up to 32, one k-block of the instruction, zeros in the padding.
//   fs16_walk_kernel<MODE>   the roles of fs_walk_kernel: a workgroup owns 64 rows (wavefront w 16 of them) and walks 64-row tiles
//                            of the other side.  Data path:
//     own rows      never touch LDS: lane (ln, q) keeps k = 8 q .. 8 q + 7 of every k-block of own row ln in registers for the
//                   whole walk (the B operand of the first product), one 16-byte global load per k-block.
//     walked tile   16-byte global loads of tile t + 1 are in flight under tile t; put() writes them row-major (pitch 2 Dk + 16
//                   bytes: the A operand is one ds_read_b128 per 16-row block and k-block) and, in the gradient modes, a second
//                   time transposed ([Dk][64 + 4] bf16).
//     S             four v_mfma_f32_16x16x32_bf16 per k-block into four interleaved accumulators; lane (ln, q) ends up with
//                   S[walked 16 s + 4 q + r][own ln], the fp32 walk's layout, so its epilogue carries over statement for statement.
//     G += a . X    the coefficients are rounded to bf16 where they sit and are the A operand: acc[0] | acc[1] fill the eight k-slots
//                   of one instruction, acc[2] | acc[3] those of a second.  The B operand presents X in the same k permutation,
//                   X[16 s + 4 q + r][16 kb + ln]: two ds_read_b64 of the transposed copy.  Two instructions per 16 columns and tile.
// No atomics: every sum has a fixed order, and the results are bit-repeatable.
#include "orx_device.h"
#include "orx_mfma16.h"

namespace {

constexpr float FS_NEG = -3.0e38f;            // "no column yet": finite, so that exp(m - m) of an empty share is 1, not NaN
constexpr int FS16_TP = 64 + 4;               // the transposed copy's pitch in bf16: rows stay 8-byte aligned for ds_read_b64

// kernels_fullsoftmax.hip fs_exp / fs_add, restated
__device__ __forceinline__ float fs_exp(float x) {
    x = fmaxf(x, -104.0f);
    const float hi = 1.44269502162933349609375f, lo = 1.92596299e-8f;
    const float t = x * hi;
    const float r = fmaf(x, lo, fmaf(x, hi, -t));
    const float e = __builtin_amdgcn_exp2f(t);
    return fmaf(e, r * 0.693147182f, e);
}

__device__ __forceinline__ void fs_add(float& s, float& c, float x) {
    const float y = x - c, t = s + y;
    c = (t - s) - y;
    s = t;
}

// one thread per eight elements of a copy: rows [0, Bp) are xq's, rows [Bp, Bp + NIp) xv's.  Dp is a multiple of 16, so a group
// of eight lies wholly inside the fp32 row or wholly in the padding
__global__ __launch_bounds__(256) void fs16_copy_kernel(FullSoftmaxArgs a) {
    const int g8 = a.Dk >> 3;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (a.Bp + a.NIp) * g8) return;
    const int64_t row = idx / g8;
    const int c = 8 * (int)(idx - row * g8);
    const bool items = row >= a.Bp;
    const int64_t r = items ? row - a.Bp : row;
    const float* src = (items ? a.xv : a.xq) + (size_t)r * a.Dp + c;
    u32x4 v = u32x4{0u, 0u, 0u, 0u};
    if (c < a.Dp) v = fs16_pack(*reinterpret_cast<const f32x4*>(src), *reinterpret_cast<const f32x4*>(src + 4));
    *reinterpret_cast<u32x4*>((items ? a.xv16 : a.xq16) + (size_t)r * a.Dk + c) = v;
}

// MODE 0: the LSE pass; 1: the gradient of the query rows; 2: of the item side.  KBMAX: the power of two at or above Dk / 32
template <int MODE, int KBMAX>
__global__ __launch_bounds__(256) void fs16_walk_kernel(FullSoftmaxArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fs16_lds[];
    const int Dk = a.Dk, nkb = Dk >> 5, ngb = a.Dp >> 4, pitch = 2 * Dk + 16, c8n = Dk >> 3;
    unsigned char* Bs = fs16_lds;                                        // [64][pitch bytes] the tile of walked rows, row-major
    unsigned short* Bt = reinterpret_cast<unsigned short*>(Bs + 64 * pitch);        // [Dk][FS16_TP] the same tile transposed (MODE 1 / 2)
    int* wkey = reinterpret_cast<int*>(Bt + (MODE == 0 ? 0 : Dk * FS16_TP));        // [64] the tile's keys
    float* wa = reinterpret_cast<float*>(wkey + 64);        // [64] MODE 0 / 1: the tile's biases;  MODE 2: its c / tot
    float* wb = wa + 64;                                    // [64] MODE 0 / 1: the tile's offsets; MODE 2: its row maxima
    float* wd = wb + 64;                                    // [64] MODE 2: the tile's label coefficients
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, ln = lane & 15;
    const unsigned short* Xo = MODE == 2 ? a.xv16 : a.xq16;
    const unsigned short* Xw = MODE == 2 ? a.xq16 : a.xv16;
    const int64_t o0 = (int64_t)blockIdx.x * 64;
    const int chunk = blockIdx.y;
    const int ntiles = (int)((MODE == 2 ? a.Bp : a.NIp) >> 6);
    const int tpc = MODE == 2 ? a.tps : a.tpi;
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
    float sa = 0.0f, sb = 0.0f, sd4 = 0.0f;
    auto fetch = [&](int tile) {
        const u32x4* src = reinterpret_cast<const u32x4*>(Xw + (size_t)tile * 64 * Dk);     // 64 c8n = 256 nkb groups of eight, contiguous
#pragma unroll
        for (int k = 0; k < KBMAX; ++k)
            if (k < nkb) stage[k] = src[tid + 256 * k];
        if (tid < 64) {
            const int64_t t = (int64_t)tile * 64 + tid;
            if (MODE == 2) { skey = a.key[t]; sa = a.cn[t]; sb = a.rmax[t]; sd4 = a.dcoef[t]; }
            else { skey = t < a.NI ? (int)t : -1; sa = a.ib[t]; sb = a.io[t]; }
        }
    };
    auto put = [&]() {
#pragma unroll
        for (int k = 0; k < KBMAX; ++k)
            if (k < nkb) {
                const int e = tid + 256 * k, r = e / c8n, c = e - r * c8n;
                *reinterpret_cast<u32x4*>(Bs + r * pitch + 16 * c) = stage[k];
                if (MODE != 0) {
                    unsigned short* col = Bt + (8 * c) * FS16_TP + r;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        col[(2 * j) * FS16_TP] = (unsigned short)(stage[k][j] & 0xffffu);
                        col[(2 * j + 1) * FS16_TP] = (unsigned short)(stage[k][j] >> 16);
                    }
                }
            }
        if (tid < 64) { wkey[tid] = skey; wa[tid] = sa; wb[tid] = sb; if (MODE == 2) wd[tid] = sd4; }
    };
    const int okey = MODE == 2 ? (o < a.NI ? (int)o : -1) : a.key[o];
    const float own_a = MODE == 1 ? a.cn[o] : (MODE == 2 ? a.ib[o] : 0.0f);       // query side: c_i / tot_i; item side: b_j
    const float own_b = MODE == 1 ? a.rmax[o] : (MODE == 2 ? a.io[o] : 0.0f);     // query side: m_i;         item side: off_j
    const float dco = MODE == 1 ? a.dcoef[o] : 0.0f;
    const float scale = a.scale;
    float m = FS_NEG, E = 0.0f, Ec = 0.0f, sd = -INFINITY;  // MODE 0
    float bsum = 0.0f, bc = 0.0f;                           // MODE 2
    int nlab = 0;                                           // MODE 2
    constexpr int GB = MODE == 0 ? 1 : 2 * KBMAX;           // 16-column blocks of G
    f32x4 G[GB];
#pragma unroll
    for (int k = 0; k < GB; ++k) G[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    const unsigned char* wrow = Bs + ln * pitch + 16 * q;
    const unsigned short* xcol = Bt + ln * FS16_TP + 4 * q;

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
        float tmax = FS_NEG, tsum = 0.0f;
        unsigned labbits = 0;                               // which of this lane's 16 walked rows is the label pair
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int base = 16 * s + 4 * q;
            const i32x4 k4 = *reinterpret_cast<const i32x4*>(wkey + base);
            const f32x4 a4 = *reinterpret_cast<const f32x4*>(wa + base);
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(wb + base);
            f32x4 d4 = f32x4{0.f, 0.f, 0.f, 0.f};
            if (MODE == 2) d4 = *reinterpret_cast<const f32x4*>(wd + base);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int kt = k4[r];
                const bool out = kt < 0 || okey < 0;
                const bool lab = !out && kt == okey;
                if (lab) labbits |= 1u << (4 * s + r);
                if (MODE == 0) {
                    const float sc = out ? -INFINITY : fmaf(scale, acc[s][r] + a4[r], b4[r]);
                    if (lab) sd = sc;
                    acc[s][r] = sc;
                    tmax = fmaxf(tmax, sc);
                } else if (MODE == 1) {
                    const float sc = fmaf(scale, acc[s][r] + a4[r], b4[r]);
                    const float pi = out ? 0.0f : own_a * fs_exp(sc - own_b);
                    acc[s][r] = lab ? dco : pi;
                } else {
                    const float sc = fmaf(scale, acc[s][r] + own_a, own_b);
                    const float pi = out ? 0.0f : a4[r] * fs_exp(sc - b4[r]);
                    const float co = lab ? d4[r] : pi;
                    acc[s][r] = co;
                    tsum += co;
                    nlab += lab ? 1 : 0;
                }
            }
        }
        if (MODE == 0) {
            const float mn = fmaxf(m, tmax);
            float e = 0.0f;
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r) e += ((labbits >> (4 * s + r)) & 1u) ? 0.0f : fs_exp(acc[s][r] - mn);
            const float f = fs_exp(m - mn);
            E *= f; Ec *= f;
            fs_add(E, Ec, e);
            m = mn;
        } else {
            if (MODE == 2) fs_add(bsum, bc, tsum);          // (the unrounded coefficients)
            // G[own 16][Dp] += bf(a)[own 16][64 walked] . X[64 walked][Dp]: k-slot j of lane group q is walked row
            // 16 (2 h + j / 4) + 4 q + j % 4 in instruction h, for the coefficients as they sit and for the transposed tile alike
            bf16x8 co[2];
#pragma unroll
            for (int h = 0; h < 2; ++h)
                co[h] = __builtin_bit_cast(bf16x8, fs16_pack(acc[2 * h], acc[2 * h + 1]));
#pragma unroll
            for (int gb = 0; gb < GB; ++gb)
                if (gb < ngb) {
                    const unsigned short* xc = xcol + 16 * gb * FS16_TP;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        u32x4 x;
                        const u32x2 x0 = *reinterpret_cast<const u32x2*>(xc + 32 * h), x1 = *reinterpret_cast<const u32x2*>(xc + 32 * h + 16);
                        x[0] = x0[0]; x[1] = x0[1]; x[2] = x1[0]; x[3] = x1[1];
                        G[gb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(co[h], __builtin_bit_cast(bf16x8, x), G[gb], 0, 0, 0);
                    }
                }
        }
        __syncthreads();                      // every wavefront is done with the tile
        if (more) put();
        __syncthreads();
    }
    const size_t prow = (size_t)chunk * (MODE == 2 ? a.NIp : a.Bp);
    if (MODE == 0) {
        // the four lane groups of a row, in lane-group order
        float M = FS_NEG, mk[4], Ek[4], sdm = -INFINITY;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            mk[k] = __shfl(m, ln + 16 * k); Ek[k] = __shfl(E, ln + 16 * k);
            sdm = fmaxf(sdm, __shfl(sd, ln + 16 * k));
            M = fmaxf(M, mk[k]);
        }
        float Es = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) Es = fmaf(Ek[k], fs_exp(mk[k] - M), Es);
        if (q == 0) { a.pm[prow + o] = M; a.pe[prow + o] = Es; a.psd[prow + o] = sdm; }
    } else {
        // the partial tiles have the fp32 walk's layout, [chunk][row][Dp]: fs_finish_kernel reads them
        float* gp = (MODE == 2 ? a.gpv : a.gpq) + (prow + (size_t)o0 + 16 * wave + 4 * q) * a.Dp + ln;
#pragma unroll
        for (int gb = 0; gb < GB; ++gb)
            if (gb < ngb) {
#pragma unroll
                for (int r = 0; r < 4; ++r) gp[(size_t)r * a.Dp + 16 * gb] = G[gb][r];
            }
        if (MODE == 2) {
            bsum += __shfl_xor(bsum, 16);
            bsum += __shfl_xor(bsum, 32);
            nlab += __shfl_xor(nlab, 16);
            nlab += __shfl_xor(nlab, 32);
            if (q == 0) { a.bpart[prow + o] = bsum; a.npart[prow + o] = nlab; }
        }
    }
}

template <int MODE>
int fs16_walk(orx_ctx* ctx, const FullSoftmaxArgs& a) {
    const dim3 g((unsigned)((MODE == 2 ? a.NIp : a.Bp) >> 6), (unsigned)(MODE == 2 ? a.ncs : a.nci));
    const size_t lds = (size_t)64 * (2 * a.Dk + 16) + (MODE == 0 ? 0 : (size_t)a.Dk * FS16_TP * 2) + 256 * sizeof(float);
    int kbmax = 1;
    while (32 * kbmax < a.Dk) kbmax *= 2;
#define ORX_FS16(KB) do { \
        ORX_ONCE_PER_DEVICE(ctx, ORX_HIP(hipFuncSetAttribute((const void*)fs16_walk_kernel<MODE, KB>, hipFuncAttributeMaxDynamicSharedMemorySize, 112 * 1024))); \
        ORX_LAUNCH(ctx, (fs16_walk_kernel<MODE, KB>), g, dim3(256), lds, a); } while (0)
    switch (kbmax) {
        case 1: ORX_FS16(1); break;
        case 2: ORX_FS16(2); break;
        case 4: ORX_FS16(4); break;
        default: ORX_FS16(8); break;
    }
#undef ORX_FS16
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

}  // namespace

// after fs_prepare_kernel and fs_items_kernel have written xq and xv: their bf16 copies
int orx_launch_fullsoftmax16_copies(orx_ctx* ctx, const FullSoftmaxArgs& a) {
    ORX_LAUNCH(ctx, fs16_copy_kernel, dim3((unsigned)(((a.Bp + a.NIp) * (a.Dk >> 3) + 255) / 256)), dim3(256), 0, a);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

int orx_launch_fullsoftmax16_walk(orx_ctx* ctx, const FullSoftmaxArgs& a, int mode) {
    return mode == 0 ? fs16_walk<0>(ctx, a) : mode == 1 ? fs16_walk<1>(ctx, a) : fs16_walk<2>(ctx, a);
}
