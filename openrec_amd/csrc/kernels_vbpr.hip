// VBPR (He & McAuley, AAAI 2016): BPR whose item vector is the latent row V[i] beside a learned projection theta_i = F[i] E of a fixed
// per-item feature row (orx_vbpr_step / orx_vbpr_loss / orx_vbpr_item_table / orx_features_project; include/openrec_hip.h has the
// semantics).  The projection has no output bias: it would cancel in every pair difference, its loss gradient is identically zero,
// and in serving it shifts all items of a user equally.
//
// Three kernels per step, none of which writes a table, so every gradient is taken on the pre-step tables:
//   vbpr_project_kernel   out[k][0:Dc] = (F[ia[k]] - F[ib[k]]) E, an fp32 MFMA product with M = rows, K = Fd, N = Dc.  A workgroup owns
//                         64 rows (wavefront w 16 of them) and all Np = Dc rounded up to 16 columns; it walks K in tiles of 32.  The A
//                         tile [64][32] is the DIFFERENCE of the two gathered rows, formed while it is staged (float4 loads when
//                         Fd % 4 == 0 and F is 16-byte aligned, scalar loads otherwise; the K tail is zero either way); the E tile
//                         [32][Np] goes through LDS with zeros beyond Dc.  v_mfma_f32_16x16x4_f32 in the layout of kernels_inbatch.hip:
//                         lane l = (q, ln) reads A[16 w + ln][16 kb + 4 q .. + 3] with one ds_read_b128 and feeds element c to step c,
//                         whose B operand is E[16 kb + 4 q + c][16 nt + ln] (row pitch Np + 4: the two lane groups of a 32-lane half
//                         sit 16 banks apart).  Np / 16 independent accumulators per wavefront.  Every product is rounded once into
//                         an fp32 fma chain of length Fd.
//   vbpr_pair_kernel      one wavefront per triplet: x_k from U[u], V[p], V[n], b and Delta_k; the per-occurrence gradient rows
//                         gu [B][gs], gi [2B][gs] (positives, then negatives; the bias gradient in column Dl), the coefficient rows
//                         R[k] = g_k U_c[u_k], the concatenated item id list and one (loss, l2) partial per wavefront.
//   vbpr_dproj_kernel     dE = df^T R over the gathered rows: M = Fd, N = Dc, the reduction over the batch.  A workgroup owns 64 rows of
//                         E and one chunk of the batch, walks it in tiles of 32 triplets -- F[p] - F[n] gathered again, [32][64] in
//                         LDS as it is loaded, R [32][Np] beside it -- and leaves a partial [Fd][Dc];
//   vbpr_dproj_finish     adds the partials in chunk order and l2_proj E.
// An id out of range sets the context's sticky index flag and is never used as an address: its row of the projection is zero, its
// triplet contributes no loss, no l2 and no gradient.  No atomics anywhere: every sum has a fixed order.
#include <algorithm>

#include "orx_device.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int VB_KT = 32;                     // K per tile
constexpr int VB_AP = VB_KT + 4;              // row pitch of the projection's A tile
constexpr int VB_DP = 64 + 4;                 // row pitch of the gradient's df tile

template <int NT>
__global__ __launch_bounds__(256) void vbpr_project_kernel(VbprProjArgs a) {
    __shared__ __attribute__((aligned(16))) float As[64 * VB_AP];
    __shared__ __attribute__((aligned(16))) float Es[VB_KT * (16 * NT + 4)];
    __shared__ int s_ia[64], s_ib[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, ln = lane & 15;
    const int Fd = a.Fd, Dc = a.Dc, Np = a.Np, ntr = Np >> 4, pe = Np + 4;
    const int64_t r0 = (int64_t)blockIdx.x * 64;
    if (tid < 64) {
        const int64_t k = r0 + tid;
        int x = -1, y = -1;                   // -1: a row of zeros
        if (k < a.n) {
            bool ok = true;
            if (a.ia) { x = a.ia[k]; ok = id_ok(x, a.NI); }
            else x = (int)(a.row0 + k);       // (the launcher has checked the range)
            if (a.ib) { y = a.ib[k]; ok = ok && id_ok(y, a.NI); }
            if (!ok) { *a.err = 1; x = -1; y = -1; }
        }
        s_ia[tid] = x; s_ib[tid] = y;
    }
    __syncthreads();
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the next tile's operands are fetched into registers while the present one is multiplied, and laid into LDS after it
    const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 pa[2], pb[2];
    float sa[8], se[2 * NT];
    const int ec = tid & 15, er0 = tid >> 4;      // E tile: this thread's column of every 16-wide column tile, its two rows
    auto fetch = [&](int k0) {
        if (a.vec) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int idx = tid + 256 * j, r = idx >> 3, c4 = idx & 7, kk = k0 + 4 * c4;
                const int x = s_ia[r], y = s_ib[r];
                const bool in = x >= 0 && kk < Fd;
                pa[j] = in ? *reinterpret_cast<const f32x4*>(a.F + (size_t)x * Fd + kk) : zero4;
                pb[j] = (in && y >= 0) ? *reinterpret_cast<const f32x4*>(a.F + (size_t)y * Fd + kk) : zero4;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int idx = tid + 256 * j, r = idx >> 5, c = idx & 31, kk = k0 + c;
                const int x = s_ia[r], y = s_ib[r];
                float v = 0.0f;
                if (x >= 0 && kk < Fd) {
                    v = a.F[(size_t)x * Fd + kk];
                    if (y >= 0) v -= a.F[(size_t)y * Fd + kk];
                }
                sa[j] = v;
            }
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int kk = k0 + er0 + 16 * h, c = 16 * nt + ec;
                se[2 * nt + h] = (nt < ntr && kk < Fd && c < Dc) ? a.E[(size_t)kk * Dc + c] : 0.0f;
            }
    };
    auto put = [&]() {
        if (a.vec) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int idx = tid + 256 * j, r = idx >> 3, c4 = idx & 7;
                *reinterpret_cast<f32x4*>(As + r * VB_AP + 4 * c4) = pa[j] - pb[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int idx = tid + 256 * j, r = idx >> 5, c = idx & 31;
                As[r * VB_AP + c] = sa[j];
            }
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (nt < ntr) Es[(er0 + 16 * h) * pe + 16 * nt + ec] = se[2 * nt + h];
    };
    fetch(0);
    put();
    __syncthreads();
    for (int k0 = 0; k0 < Fd; k0 += VB_KT) {
        const bool more = k0 + VB_KT < Fd;
        if (more) fetch(k0 + VB_KT);
#pragma unroll
        for (int kb = 0; kb < VB_KT / 16; ++kb) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(As + (16 * wave + ln) * VB_AP + 16 * kb + 4 * q);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float* er = Es + (16 * kb + 4 * q + c) * pe + ln;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    if (nt < ntr) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c], er[16 * nt], acc[nt], 0, 0, 0);
            }
        }
        __syncthreads();                      // every wavefront is done with the tile
        if (more) put();
        __syncthreads();
    }
    // acc[nt][r] = out[row 16 wave + 4 q + r][column 16 nt + ln]
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        if (nt < ntr) {
            const int c = 16 * nt + ln;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * wave + 4 * q + r;
                const int64_t k = r0 + row;
                if (k < a.n && c < Dc) a.out[(size_t)k * a.out_stride + a.out_col0 + c] = s_ia[row] >= 0 ? acc[nt][r] : 0.0f;
            }
        }
    }
}

// x: term = -log_sigmoid(max(x, -30)), sig = sigmoid(-x) [x >= -30] -- the expressions of score<ORX_BPR> (orx_device.h)
__device__ __forceinline__ void vb_logsig(float x, float& term, float& sig) {
    const float m = fmaxf(x, -30.0f);
    const float e = __expf(-fabsf(m));
    term = fmaxf(-m, 0.0f) + log1p_unit(e);
    const float s = (x >= 0.0f) ? e / (1.0f + e) : 1.0f / (1.0f + e);
    sig = (x >= -30.0f) ? s : 0.0f;
}

template <bool GRAD>
__global__ __launch_bounds__(256) void vbpr_pair_kernel(VbprPairArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Dl = a.Dl, Dc = a.Dc, D = Dl + Dc;
    const size_t gs = (size_t)a.gs;
    const int64_t wave_global = (int64_t)blockIdx.x * 4 + wave;
    const int64_t stride = (int64_t)gridDim.x * 4;
    float loss_acc = 0.0f, sq_acc = 0.0f;
    for (int64_t t = wave_global; t < a.B; t += stride) {
        const int u = a.uid[t], p = a.pid[t], n = a.nid[t];
        const bool ok = id_ok(u, a.NU) && id_ok(p, a.NI) && id_ok(n, a.NI);       // (wave-uniform)
        if (!ok && lane == 0) *a.err = 1;
        const float* ur = a.U + (size_t)(ok ? u : 0) * D;
        const float* pr = a.V + (size_t)(ok ? p : 0) * Dl;
        const float* nr = a.V + (size_t)(ok ? n : 0) * Dl;
        const float* dr = a.delta + (size_t)t * Dc;
        float part = 0.0f, sq = 0.0f;
        if (ok)
            for (int e = lane; e < D; e += 64) {
                const float x = ur[e];
                if (e < Dl) {
                    const float y = pr[e], z = nr[e];
                    part = fmaf(x, y - z, part);
                    sq += x * x + y * y + z * z;
                } else {
                    part = fmaf(x, dr[e - Dl], part);
                    sq += x * x;
                }
            }
        float xk = wave_sum(part);
        if (ok && a.b) xk += a.b[p] - a.b[n];
        const float c = ok ? (a.wt ? a.wt[t] : 1.0f) * a.invB : 0.0f;
        float term, sig;
        vb_logsig(xk, term, sig);
        if (ok) {
            sq_acc += sq;
            if (lane == 0) loss_acc += c * term;
        }
        if (GRAD) {
            const float g = ok ? -c * sig : 0.0f;
            float* gur = a.gu + (size_t)t * gs;
            float* gpr = a.gi + (size_t)t * gs;
            float* gnr = a.gi + ((size_t)a.B + (size_t)t) * gs;
            for (int e = lane; e < D; e += 64) {
                const float x = ok ? ur[e] : 0.0f;
                if (e < Dl) {
                    const float y = ok ? pr[e] : 0.0f, z = ok ? nr[e] : 0.0f;
                    gur[e] = fmaf(g, y - z, a.l2w * x);
                    gpr[e] = fmaf(g, x, a.l2w * y);
                    gnr[e] = fmaf(-g, x, a.l2w * z);
                } else {
                    gur[e] = ok ? fmaf(g, dr[e - Dl], a.l2w * x) : 0.0f;
                    a.R[(size_t)t * Dc + (e - Dl)] = g * x;
                }
            }
            if (lane == 0) {
                gpr[Dl] = g; gnr[Dl] = -g;
                a.list[t] = p; a.list[a.B + t] = n;
            }
        }
    }
    const float ls = wave_sum(loss_acc);
    const float sqs = wave_sum(sq_acc);
    if (lane == 0) {
        float2 v; v.x = ls; v.y = 0.5f * sqs;
        *reinterpret_cast<float2*>(a.partial + 2 * wave_global) = v;
    }
}

template <int NT>
__global__ __launch_bounds__(256) void vbpr_dproj_kernel(VbprDprojArgs a) {
    __shared__ __attribute__((aligned(16))) float Ds[VB_KT * VB_DP];
    __shared__ __attribute__((aligned(16))) float Rs[VB_KT * (16 * NT + 4)];
    __shared__ int s_p[2][VB_KT], s_n[2][VB_KT];              // the ids of the tile being fetched and of the one after it
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, ln = lane & 15;
    const int Fd = a.Fd, Dc = a.Dc, Np = a.Np, ntr = Np >> 4, pr = Np + 4;
    const int f0 = blockIdx.x * 64, ch = blockIdx.y;
    const int64_t kbeg = (int64_t)ch * a.chunk_rows;
    const int64_t kend = kbeg + a.chunk_rows < a.B ? kbeg + a.chunk_rows : a.B;
    const int ntiles = (int)((kend - kbeg + VB_KT - 1) / VB_KT);
    const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = zero4;
    int idp = -1, idn = -1;
    auto fetch_ids = [&](int tile) {          // threads 0 .. 31: the ids of one tile's triplets; -1: a row of zeros
        idp = -1; idn = -1;
        const int64_t k = kbeg + (int64_t)tile * VB_KT + tid;
        if (tid < VB_KT && tile < ntiles && k < kend) {
            idp = a.pid[k]; idn = a.nid[k];
            if (!id_ok(idp, a.NI) || !id_ok(idn, a.NI)) { idp = -1; idn = -1; }
        }
    };
    auto put_ids = [&](int buf) { if (tid < VB_KT) { s_p[buf][tid] = idp; s_n[buf][tid] = idn; } };
    // the next tile's rows are fetched into registers while the present one is multiplied, and laid into LDS after it
    f32x4 pa[2], pb[2];
    float sa[8], sr[2 * NT];
    const int rc = tid & 15, rr0 = tid >> 4;      // R tile: this thread's column of every 16-wide column tile, its two rows
    auto fetch = [&](int tile, int buf) {
        if (a.vec) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int idx = tid + 256 * j, r = idx >> 4, c4 = idx & 15, f = f0 + 4 * c4;
                const int p = s_p[buf][r], n = s_n[buf][r];
                const bool in = p >= 0 && f < Fd;
                pa[j] = in ? *reinterpret_cast<const f32x4*>(a.F + (size_t)p * Fd + f) : zero4;
                pb[j] = in ? *reinterpret_cast<const f32x4*>(a.F + (size_t)n * Fd + f) : zero4;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int idx = tid + 256 * j, r = idx >> 6, c = idx & 63, f = f0 + c;
                const int p = s_p[buf][r], n = s_n[buf][r];
                sa[j] = (p >= 0 && f < Fd) ? a.F[(size_t)p * Fd + f] - a.F[(size_t)n * Fd + f] : 0.0f;
            }
        }
        const int64_t k0 = kbeg + (int64_t)tile * VB_KT;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int64_t k = k0 + rr0 + 16 * h;
                const int c = 16 * nt + rc;
                sr[2 * nt + h] = (nt < ntr && k < kend && c < Dc) ? a.R[(size_t)k * Dc + c] : 0.0f;
            }
    };
    auto put = [&]() {
        if (a.vec) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int idx = tid + 256 * j, r = idx >> 4, c4 = idx & 15;
                *reinterpret_cast<f32x4*>(Ds + r * VB_DP + 4 * c4) = pa[j] - pb[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int idx = tid + 256 * j, r = idx >> 6, c = idx & 63;
                Ds[r * VB_DP + c] = sa[j];
            }
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (nt < ntr) Rs[(rr0 + 16 * h) * pr + 16 * nt + rc] = sr[2 * nt + h];
    };
    fetch_ids(0); put_ids(0);
    fetch_ids(1); put_ids(1);
    __syncthreads();
    fetch(0, 0);
    put();
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
        const bool more = t + 1 < ntiles;
        if (more) fetch(t + 1, (t + 1) & 1);
        fetch_ids(t + 2);
#pragma unroll
        for (int kb = 0; kb < VB_KT / 16; ++kb)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int kk = 16 * kb + 4 * q + c;
                const float av = Ds[kk * VB_DP + 16 * wave + ln];
                const float* rr = Rs + kk * pr + ln;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    if (nt < ntr) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, rr[16 * nt], acc[nt], 0, 0, 0);
            }
        __syncthreads();                      // every wavefront is done with the tile, and with the ids of tile t + 1
        if (more) put();
        put_ids(t & 1);                       // (the ids of tile t + 2 take the place of tile t's)
        __syncthreads();
    }
    float* part = a.part + (size_t)ch * Fd * Dc;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        if (nt < ntr) {
            const int c = 16 * nt + ln;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = f0 + 16 * wave + 4 * q + r;
                if (f < Fd && c < Dc) part[(size_t)f * Dc + c] = acc[nt][r];
            }
        }
    }
}

// one thread per element of E: the chunks in chunk order, then the l2 term
__global__ __launch_bounds__(256) void vbpr_dproj_finish_kernel(VbprDprojArgs a) {
    const int64_t n = (int64_t)a.Fd * a.Dc;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.0f;
    for (int ch = 0; ch < a.nch; ++ch) s += a.part[(size_t)ch * n + i];
    a.dE[i] = fmaf(a.l2p, a.E[i], s);
}

__global__ __launch_bounds__(256) void vbpr_copy_cols_kernel(const float* V, int Dl, float* W, int D, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t r = i / Dl;
    const int c = (int)(i - r * Dl);
    W[(size_t)r * D + c] = V[i];
}

inline int64_t vb_pair_blocks(int num_cu, int64_t B) {
    int64_t g = (B + 3) / 4;
    const int64_t cap = (int64_t)num_cu * 16;
    if (g > cap) g = cap;
    return g < 1 ? 1 : g;
}

inline int vb_nt(int Np) {
    int nt = 1;
    while (16 * nt < Np) nt *= 2;
    return nt;
}

}  // namespace

int orx_vbpr_nwaves(orx_ctx* ctx, int64_t B) { return (int)(vb_pair_blocks(ctx->num_cu, B) * 4); }

// what the launcher of the projection gradient does for (B, Fd, Dc): rows of the batch per chunk, chunks, padded Dc, rows of E per
// workgroup.  Its own chunking aims at 1024 workgroups and keeps at least 256 triplets per chunk.
void orx_vbpr_plan(int64_t B, int32_t Fd, int32_t Dc, int32_t batch_chunk, int32_t out[4]) {
    const int64_t ftiles = (Fd + 63) / 64;
    int64_t cr;
    if (batch_chunk > 0) cr = batch_chunk;
    else {
        const int64_t want = std::max<int64_t>(1, 1024 / ftiles);
        cr = std::max<int64_t>(256, (((B + want - 1) / want) + 63) & ~(int64_t)63);
    }
    out[0] = (int32_t)cr;
    out[1] = (int32_t)std::max<int64_t>(1, (B + cr - 1) / cr);
    out[2] = (Dc + 15) & ~15;
    out[3] = 64;
}

int orx_launch_vbpr_project(orx_ctx* ctx, const VbprProjArgs& a) {
    if (a.n == 0) return ORX_OK;
    ProfScope ps(ctx, ORX_K_GEMM);
    const dim3 g((unsigned)((a.n + 63) / 64));
    switch (vb_nt(a.Np)) {
        case 1: ORX_LAUNCH(ctx, vbpr_project_kernel<1>, g, dim3(256), 0, a); break;
        case 2: ORX_LAUNCH(ctx, vbpr_project_kernel<2>, g, dim3(256), 0, a); break;
        case 4: ORX_LAUNCH(ctx, vbpr_project_kernel<4>, g, dim3(256), 0, a); break;
        default: ORX_LAUNCH(ctx, vbpr_project_kernel<8>, g, dim3(256), 0, a); break;
    }
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

// grads == false: the loss-only instantiation (a.gu / a.gi / a.R / a.list are not touched)
int orx_launch_vbpr_pairs(orx_ctx* ctx, bool grads, const VbprPairArgs& a) {
    ProfScope ps(ctx, ORX_K_FUSED);
    const dim3 g((unsigned)vb_pair_blocks(ctx->num_cu, a.B));
    if (grads) ORX_LAUNCH(ctx, vbpr_pair_kernel<true>, g, dim3(256), 0, a);
    else ORX_LAUNCH(ctx, vbpr_pair_kernel<false>, g, dim3(256), 0, a);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

int orx_launch_vbpr_dproj(orx_ctx* ctx, const VbprDprojArgs& a) {
    {
        ProfScope ps(ctx, ORX_K_GEMM);
        const dim3 g((unsigned)((a.Fd + 63) / 64), (unsigned)a.nch);
        switch (vb_nt(a.Np)) {
            case 1: ORX_LAUNCH(ctx, vbpr_dproj_kernel<1>, g, dim3(256), 0, a); break;
            case 2: ORX_LAUNCH(ctx, vbpr_dproj_kernel<2>, g, dim3(256), 0, a); break;
            case 4: ORX_LAUNCH(ctx, vbpr_dproj_kernel<4>, g, dim3(256), 0, a); break;
            default: ORX_LAUNCH(ctx, vbpr_dproj_kernel<8>, g, dim3(256), 0, a); break;
        }
        ORX_HIP(hipGetLastError());
    }
    ProfScope ps(ctx, ORX_K_REDUCE);
    ORX_LAUNCH(ctx, vbpr_dproj_finish_kernel, dim3((unsigned)(((int64_t)a.Fd * a.Dc + 255) / 256)), dim3(256), 0, a);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

int orx_launch_vbpr_copy_cols(orx_ctx* ctx, const float* V, int Dl, float* W, int D, int64_t nrows) {
    const int64_t n = nrows * Dl;
    if (n == 0) return ORX_OK;
    ORX_LAUNCH(ctx, vbpr_copy_cols_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, V, Dl, W, D, n);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}
