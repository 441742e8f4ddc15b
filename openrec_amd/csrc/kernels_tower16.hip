// The dense tower with bf16 operands on the matrix cores (ORX_TOWER_BF16; include/openrec_hip.h has the rounded semantics, DESIGN
// 4.5x.1 the construction).  kernels_tower.hip keeps the input, the finishing pass and the fp32 layers; this file holds the layers'
// products around v_mfma_f32_16x16x32_bf16.  Operands are rounded to nearest even once, where they enter LDS or the bf16 copies;
// accumulators, biases, masks, the l2 terms and every stored activation and gradient stay fp32.
//
//   tw16_cast_kernel       one launch per call: for every layer the two bf16 copies of W_l [K][N], zero-padded to the instruction's
//                          multiples -- wk16 [N up to 16][K up to 32], k contiguous (the forward's B operand), and wn16
//                          [K up to 16][N up to 32], n contiguous (the B operand of g_l = gm W_l^T).  No product loop reads W itself.
//   tw16_rows_kernel<BWD>  the two products that are parallel over the batch, one launch per layer: a workgroup owns 16 rows (256
//                          workgroups at B = 4096) and the full output width, wavefront w the 16-column blocks w, w + 4, ...
//     rows       the tile is rounded to bf16 on its way into LDS, [16][C up to 32] (C: the contraction's width), once: x_l for the
//                forward; gm = g_{l+1} .* (x_{l+1} > 0) for the backward.  The A operand is one ds_read_b128 per k-block.
//     W          the bf16 copy goes through LDS in slabs of one k-block (32 wide, every output column), 16-byte global loads of
//                slab s + 1 in flight under the products of slab s, two LDS buffers, one barrier per slab.  Pitch 80 bytes.
//     epilogue   forward: + c_l, relu, fp32 stores.  Backward: + l2x x_0 (l = 0), fp32 stores.
//                An output element is one accumulator chain over the k-blocks in order: its bits depend on its own row and the
//                widths alone.
//   tw16_dw_kernel         dW_l = x_l^T gm, the contraction over the batch: a workgroup owns one 64 x 64 tile of dW_l and one batch
//                          chunk (grid: k blocks x n blocks x chunks; orx_tower16_plan).  Per 64 rows of the batch, x_l and gm are
//                          staged TRANSPOSED in LDS ([64 columns][64 rows] bf16, pitch 144 bytes), so a lane's eight batch entries
//                          are one ds_read_b128 for either operand.  The tile stays in accumulators over the whole chunk and is
//                          written once, to the chunk's partial ([chunk][K N], tower_finish_kernel's layout).  The workgroups of
//                          k block 0 also sum the UNROUNDED gm of their 64 columns: four row groups (rows 16 g .. 16 g + 15 of
//                          every tile, in tile and row order) combined in group order -> the chunk's partial of dc_l.
// No atomics: every sum has a fixed order that (B, the widths) determine, and the results are bit-repeatable.  Every global access is
// guarded by the true sizes; the LDS tiles and the bf16 copies are zero beyond them, so the products need no guards.
#include <algorithm>

#include "orx_device.h"
#include "orx_mfma16.h"
#include "orx_tower_device.h"

namespace {

constexpr int TW16_ROWS = 16;                 // batch rows per workgroup of tw16_rows_kernel
constexpr int TW16_WP = 64 + 16;              // a slab row: 32 bf16 and 16 bytes of padding
constexpr int TW16_TP = 128 + 16;             // a row of the transposed tiles: 64 bf16 and 16 bytes of padding

__device__ __forceinline__ u32x4 tw16_pack8(const float* v) {
    return fs16_pack(f32x4{v[0], v[1], v[2], v[3]}, f32x4{v[4], v[5], v[6], v[7]});
}

// blockIdx.y: the layer; one thread per eight elements of a copy
__global__ __launch_bounds__(256) void tw16_cast_kernel(TowerArgs t) {
    const int l = blockIdx.y;
    const int K = t.w[l], N = t.w[l + 1];
    const int Kp32 = (K + 31) & ~31, Np16 = (N + 15) & ~15, Kp16 = (K + 15) & ~15, Np32 = (N + 31) & ~31;
    const float* W = t.W[l];
    const int gk = Np16 * (Kp32 >> 3), gn = t.wn16[l] ? Kp16 * (Np32 >> 3) : 0;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    float v[8];
    if (idx < gk) {                             // wk16[n][k8 .. k8 + 7]: neighbouring lanes read neighbouring n
        const int k8 = 8 * (idx / Np16), n = idx - (idx / Np16) * Np16;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (n < N && k8 + j < K) ? W[(size_t)(k8 + j) * N + n] : 0.0f;
        *reinterpret_cast<u32x4*>(t.wk16[l] + (size_t)n * Kp32 + k8) = tw16_pack8(v);
    } else if (idx < gk + gn) {                 // wn16[k][n8 .. n8 + 7]
        const int e = idx - gk, g8 = Np32 >> 3;
        const int k = e / g8, n8 = 8 * (e - k * g8);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (k < K && n8 + j < N) ? W[(size_t)k * N + n8 + j] : 0.0f;
        *reinterpret_cast<u32x4*>(t.wn16[l] + (size_t)k * Np32 + n8) = tw16_pack8(v);
    }
}

// BWD false: x_{l+1} = act(x_l W_l + c_l);  true: g_l = gm W_l^T (+ l2x x_0).  C: the contraction's width, O: the output's
template <bool BWD>
__global__ __launch_bounds__(256) void tw16_rows_kernel(TowerArgs t, int l) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tw16_lds[];
    const int C = BWD ? t.w[l + 1] : t.w[l], O = BWD ? t.w[l] : t.w[l + 1];
    const int Cp = (C + 31) & ~31, Op = (O + 15) & ~15, nkb = Cp >> 5, nob = Op >> 4, xpitch = 2 * Cp + 16;
    unsigned char* Xs = tw16_lds;                               // [16][xpitch bytes] the rows, bf16
    unsigned char* Ws = Xs + TW16_ROWS * xpitch;                // [2][Op][TW16_WP bytes] the slabs of the bf16 copy
    const unsigned short* W16 = BWD ? t.wn16[l] : t.wk16[l];    // [Op][Cp]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, ln = lane & 15;
    const int64_t row0 = (int64_t)blockIdx.x * TW16_ROWS;
    const bool relu = l + 1 < t.L || t.relu_last;
    const float* X = t.x[l];
    const int ldx = t.ldx[l];
    float* Y = t.x[l + 1];
    const int ldy = t.ldx[l + 1];
    const float* GY = t.g[l + 1];
    const int ldgy = t.ldg[l + 1];

    u32x4 stage[4];
    auto fetch = [&](int kb) {                  // 4 Op groups of 16 bytes: row n, bytes 16 c of the k-block
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = tid + 256 * j;
            if (e < 4 * Op) stage[j] = *reinterpret_cast<const u32x4*>(W16 + (size_t)(e >> 2) * Cp + 32 * kb + 8 * (e & 3));
        }
    };
    auto put = [&](int buf) {
        unsigned char* dst = Ws + buf * Op * TW16_WP;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = tid + 256 * j;
            if (e < 4 * Op) *reinterpret_cast<u32x4*>(dst + (e >> 2) * TW16_WP + 16 * (e & 3)) = stage[j];
        }
    };
    fetch(0);
    // the rows, rounded once
    const int c8n = Cp >> 3;
    for (int e = tid; e < TW16_ROWS * c8n; e += 256) {
        const int r = e / c8n, c = 8 * (e - r * c8n);
        const int64_t row = row0 + r;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float x = 0.0f;
            if (row < t.B && c + j < C) {
                if (BWD) {
                    x = GY[(size_t)row * ldgy + c + j];
                    if (relu && !(Y[(size_t)row * ldy + c + j] > 0.0f)) x = 0.0f;
                } else {
                    x = X[(size_t)row * ldx + c + j];
                }
            }
            v[j] = x;
        }
        *reinterpret_cast<u32x4*>(Xs + r * xpitch + 2 * c) = tw16_pack8(v);
    }
    put(0);
    __syncthreads();

    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // A: rows[ln][32 kb + 8 q ..];  B: W16[16 ob + ln][32 kb + 8 q ..]
    const unsigned char* arow = Xs + ln * xpitch + 16 * q;
    for (int kb = 0; kb < nkb; ++kb) {
        const bool more = kb + 1 < nkb;
        if (more) fetch(kb + 1);
        const bf16x8 av = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(arow + 64 * kb));
        const unsigned char* brow = Ws + (kb & 1) * Op * TW16_WP + ln * TW16_WP + 16 * q;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ob = wave + 4 * j;
            if (ob < nob) {
                const bf16x8 bv = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(brow + 16 * ob * TW16_WP));
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc[j], 0, 0, 0);
            }
        }
        if (more) put((kb + 1) & 1);            // (the other buffer: every wavefront left it at the last barrier)
        __syncthreads();
    }
    // acc[j][r] = (row 4 q + r, column 16 ob + ln)
    const float* cb = t.c[l];
    float* GX = t.g[l];
    const int ldgx = t.ldg[l];
    const float l2x = t.l2x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int o = 16 * (wave + 4 * j) + ln;
        if (o < O) {
            const float bias = (!BWD && cb) ? cb[o] : 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = row0 + 4 * q + r;
                if (row < t.B) {
                    if (BWD) {
                        GX[(size_t)row * ldgx + o] = l == 0 ? tw_l2_add(l2x, X[(size_t)row * ldx + o], acc[j][r]) : acc[j][r];
                    } else {
                        float v = acc[j][r] + bias;
                        if (relu) v = v > 0.0f ? v : 0.0f;
                        Y[(size_t)row * ldy + o] = v;
                    }
                }
            }
        }
    }
}

// grid (k blocks, n blocks, chunks): the 64 x 64 tile (64 blockIdx.x, 64 blockIdx.y) of dW_l over the rows of chunk blockIdx.z
__global__ __launch_bounds__(256) void tw16_dw_kernel(TowerArgs t, int l) {
    __shared__ __attribute__((aligned(16))) unsigned char XT[64 * TW16_TP];     // [64 k][64 rows] bf16
    __shared__ __attribute__((aligned(16))) unsigned char GT[64 * TW16_TP];     // [64 n][64 rows] bf16
    __shared__ float dcs[4][64];
    const int K = t.w[l], N = t.w[l + 1];
    const int k0 = 64 * blockIdx.x, n0 = 64 * blockIdx.y, chunk = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, ln = lane & 15;
    const bool relu = l + 1 < t.L || t.relu_last;
    const float* X = t.x[l];
    const int ldx = t.ldx[l];
    const float* Y = t.x[l + 1];
    const int ldy = t.ldx[l + 1];
    const float* GY = t.g[l + 1];
    const int ldgy = t.ldg[l + 1];
    const int64_t ntiles = (t.B + 63) >> 6;
    const int64_t t_beg = (int64_t)chunk * t.tpc, t_end = std::min<int64_t>(t_beg + t.tpc, ntiles);
    // this thread stages column `lane` of either block, rows 16 wave .. 16 wave + 15 of every tile
    const bool kx = k0 + lane < K, nx = n0 + lane < N;
    float xv[16], gv[16], dc = 0.0f;
    auto fetch = [&](int64_t tile) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int64_t row = tile * 64 + 16 * wave + j;
            const bool live = row < t.B;
            xv[j] = (live && kx) ? X[(size_t)row * ldx + k0 + lane] : 0.0f;
            float g = 0.0f;
            if (live && nx) {
                g = GY[(size_t)row * ldgy + n0 + lane];
                if (relu && !(Y[(size_t)row * ldy + n0 + lane] > 0.0f)) g = 0.0f;
            }
            gv[j] = g;
        }
    };
    auto put = [&]() {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<u32x4*>(XT + lane * TW16_TP + 32 * wave + 16 * h) = tw16_pack8(xv + 8 * h);
            *reinterpret_cast<u32x4*>(GT + lane * TW16_TP + 32 * wave + 16 * h) = tw16_pack8(gv + 8 * h);
        }
        if (blockIdx.x == 0) {                  // (the unrounded gm; only k block 0 writes dc)
#pragma unroll
            for (int j = 0; j < 16; ++j) dc += gv[j];
        }
    };
    f32x4 acc[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool mine = k0 + 16 * wave < K;       // wavefront w owns rows k0 + 16 w .. + 15 of the tile
    // A: x^T[k0 + 16 wave + ln][rows 32 s + 8 q ..];  B: gm^T[n0 + 16 nb + ln][rows 32 s + 8 q ..]
    const unsigned char* arow = XT + (16 * wave + ln) * TW16_TP + 16 * q;
    const unsigned char* brow = GT + ln * TW16_TP + 16 * q;
    fetch(t_beg);
    put();
    __syncthreads();
    for (int64_t tile = t_beg; tile < t_end; ++tile) {
        const bool more = tile + 1 < t_end;
        if (more) fetch(tile + 1);
        if (mine) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const bf16x8 av = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(arow + 64 * s));
#pragma unroll
                for (int nb = 0; nb < 4; ++nb)
                    if (n0 + 16 * nb < N) {
                        const bf16x8 bv = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(brow + 16 * nb * TW16_TP + 64 * s));
                        acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc[nb], 0, 0, 0);
                    }
            }
        }
        __syncthreads();                        // every wavefront is done with the tile
        if (more) put();
        __syncthreads();
    }
    // acc[nb][r] = dW[k0 + 16 wave + 4 q + r][n0 + 16 nb + ln]: the chunk's partial, written once
    float* pw = t.pw[l] + (size_t)chunk * K * N;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
        const int n = n0 + 16 * nb + ln;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = k0 + 16 * wave + 4 * q + r;
            if (k < K && n < N) pw[(size_t)k * N + n] = acc[nb][r];
        }
    }
    if (blockIdx.x == 0) {                      // dc: the four row groups in group order
        dcs[wave][lane] = dc;
        __syncthreads();
        if (tid < 64 && n0 + tid < N) t.pc[l][(size_t)chunk * N + n0 + tid] = ((dcs[0][tid] + dcs[1][tid]) + dcs[2][tid]) + dcs[3][tid];
    }
}

inline size_t tw16_rows_lds(int C, int O) {
    return (size_t)TW16_ROWS * (2 * ((C + 31) & ~31) + 16) + (size_t)2 * ((O + 15) & ~15) * TW16_WP;
}

template <bool BWD>
int tw16_rows(orx_ctx* ctx, const TowerArgs& a, int l) {
    ORX_ONCE_PER_DEVICE(ctx, ORX_HIP(hipFuncSetAttribute((const void*)tw16_rows_kernel<BWD>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024)));
    ProfScope ps(ctx, ORX_K_GEMM);
    const size_t lds = BWD ? tw16_rows_lds(a.w[l + 1], a.w[l]) : tw16_rows_lds(a.w[l], a.w[l + 1]);
    ORX_LAUNCH(ctx, tw16_rows_kernel<BWD>, dim3((unsigned)((a.B + TW16_ROWS - 1) / TW16_ROWS)), dim3(256), lds, a, l);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

}  // namespace

// at most 32 batch chunks of 64-row tiles: the partials of a 256 x 256 layer are at most 8 MiB + 32 KB (dW and dc) whatever B is, and at B = 4096 its
// dW grid is 4 x 4 tiles x 32 chunks = 512 workgroups
void orx_tower16_plan(int64_t B, int* nch, int* tpc) {
    const int64_t ntiles = std::max<int64_t>(1, (B + 63) >> 6);
    const int64_t t = (ntiles + 31) / 32;
    *tpc = (int)t;
    *nch = (int)((ntiles + t - 1) / t);
}

int orx_tower16_tile() { return TW16_ROWS; }

int orx_launch_tower16_cast(orx_ctx* ctx, const TowerArgs& a) {
    if (a.B == 0) return ORX_OK;
    int most = 0;
    for (int l = 0; l < a.L; ++l) {
        const int K = a.w[l], N = a.w[l + 1];
        most = std::max(most, ((N + 15) & ~15) * (((K + 31) & ~31) >> 3) + ((K + 15) & ~15) * (((N + 31) & ~31) >> 3));
    }
    ProfScope ps(ctx, ORX_K_FUSED);
    ORX_LAUNCH(ctx, tw16_cast_kernel, dim3((unsigned)((most + 255) / 256), (unsigned)a.L), dim3(256), 0, a);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

int orx_launch_tower16_forward(orx_ctx* ctx, const TowerArgs& a) {
    if (a.B == 0) return ORX_OK;
    for (int l = 0; l < a.L; ++l) CHECK(tw16_rows<false>(ctx, a, l));
    return ORX_OK;
}

int orx_launch_tower16_backward(orx_ctx* ctx, const TowerArgs& a) {
    if (a.B == 0) return ORX_OK;
    for (int l = a.L - 1; l >= 0; --l) {
        if (a.g[l]) CHECK(tw16_rows<true>(ctx, a, l));
        if (a.pw[l]) {
            ProfScope ps(ctx, ORX_K_GEMM);
            const dim3 g((unsigned)((a.w[l] + 63) >> 6), (unsigned)((a.w[l + 1] + 63) >> 6), (unsigned)a.nch);
            ORX_LAUNCH(ctx, tw16_dw_kernel, g, dim3(256), 0, a, l);
            ORX_HIP(hipGetLastError());
        }
    }
    return ORX_OK;
}
