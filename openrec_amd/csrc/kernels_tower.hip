// The dense tower between the pooled history and the full softmax's query (orx_tower_step / orx_tower_loss / orx_tower_query,
// include/openrec_hip.h has the semantics):
//
//   x0_i = [ S_1[f_1[i]] | ... | S_m[f_m[i]] | pool(H[bag_i]) ];   x_{l+1} = act(x_l W_l + c_l);   q_i = x_L
//
// Four kernels, none of which writes a table:
//   tower_input_kernel     one wavefront per sample.  The side rows are gathered and the history is pooled into ONE row of x0.  The
//                          pool is bag_pool_kernel's walk restated (kernels_bag.hip): the same lane groups, the same order of the
//                          additions, c_i rounded once and the product once -- a bag's pooled bits are orx_bag_pool's.  It writes what
//                          the pool writes: uid'[i] = i (-1: a dead sample), c_i, the owner of every list position.  (|x0_i|^2, the
//                          query side's l2 term, is summed by the full softmax's prepare pass beside |V[pid_i]|^2, lane by lane as
//                          it sums |u_i|^2 in the forms without a tower.)  A sample with a bad id -- in its bag or in a side list --
//                          is dead as a whole: x0_i = +0, c_i = 0, uid' = -1, the index flag raised; no id is ever an address.
//   tower_forward_kernel   x_{l+1} = act(x_l W_l + c_l) on 64-row batch tiles; a workgroup covers its tile's full output width (at
//                          most 256), wavefront w rows 16 w .. 16 w + 15.  v_mfma_f32_16x16x4_f32, exact fp32: an output element is one
//                          fmaf chain over k = 0, 4, 8, .. -- the order depends on the widths alone, so a row's bits are the same in
//                          any batch and at any position of it.
//   tower_backward_kernel  per layer, last to first; a workgroup owns one batch chunk (tpc tiles).  Per tile the masked gradient
//                          gm = g_{l+1} .* (x_{l+1} > 0) and x_l are put in LDS once; from there g_l = gm W_l^T (+ l2x x_0 for l = 0),
//                          and the tile's dW_l = x_l^T gm and dc_l = colsum(gm), which are added to the chunk's partials in tile order
//                          by the one workgroup that owns them.  relu'(0) = 0.
//   tower_finish_kernel    one launch: every layer's partials in chunk order, + l2m * (W, c) -> the dense gradients.
// No atomics: every sum has a fixed order.  Every access is guarded by the true sizes (rows < B, columns < the widths); the LDS tiles
// are zero beyond them, so the products need no guards of their own.
#include <algorithm>

#include "orx_device.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int TW_UN = 4;           // row-load instructions in flight per wavefront of the pool (bag_pool_kernel's BAG_UN)
constexpr int TW_NB = ORX_TOWER_WIDTH / 16;

struct TwSpan { int64_t lo; int64_t len; bool bad; };

__device__ __forceinline__ TwSpan tw_span(const BagArgs& a, int64_t i) {
    const int64_t lo = a.ptr[i], hi = a.ptr[i + 1];
    TwSpan s;
    s.bad = lo < 0 || hi < lo || hi > a.n || (i == 0 && lo != 0) || (i == a.B - 1 && hi != a.n);
    s.lo = lo; s.len = s.bad ? 0 : hi - lo;
    return s;
}

// ids [c0, c0 + 64) of the bag, one per lane: -1 where the bag ends or the id lies outside H (*bad then); the owner of the position
__device__ __forceinline__ int tw_ids(const BagArgs& a, const TwSpan& sp, int64_t i, int64_t c0, int lane, bool* bad) {
    int id = -1;
    if (c0 + lane < sp.len) {
        const int64_t e = sp.lo + c0 + lane;
        id = a.items[e];
        if (!id_ok(id, a.rows)) { id = -1; *bad = true; }
        if (a.owner) a.owner[e] = (int32_t)i;
    }
    return id;
}

// LPR > 0: bag_pool_kernel<LPR>'s walk (H.dim % 4 == 0, H on 16 bytes); 0: bag_pool_generic_kernel's
template <int LPR>
__global__ __launch_bounds__(256) void tower_input_kernel(TowerArgs t) {
    const BagArgs& a = t.bag;
    constexpr int G = LPR > 0 ? 64 / LPR : 1, P = LPR > 0 ? LPR : 1;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.B) return;
    bool bad = false;
    int sid[ORX_TOWER_SIDE];
#pragma unroll
    for (int j = 0; j < ORX_TOWER_SIDE; ++j) {
        sid[j] = 0;
        if (j < t.m) {
            sid[j] = t.f[j][i];
            if (!id_ok(sid[j], t.srows[j])) { sid[j] = 0; bad = true; }
        }
    }
    const TwSpan sp = tw_span(a, i);
    bad = bad || sp.bad;
    const int sub = lane % P, grp = lane / P, col = 4 * sub;
    const bool act = col < a.D;
    f4 s4 = {0.f, 0.f, 0.f, 0.f};
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t c0 = 0; c0 < sp.len; c0 += 64) {
        const int cnt = (int)(sp.len - c0 < 64 ? sp.len - c0 : 64);
        const int mine = tw_ids(a, sp, i, c0, lane, &bad);
        if (LPR > 0) {
            for (int j0 = 0; j0 * G < cnt; j0 += TW_UN) {
                f4 x[TW_UN];
#pragma unroll
                for (int u = 0; u < TW_UN; ++u) {
                    const int k = (j0 + u) * G + grp;
                    const int id = __shfl(mine, k);
                    x[u] = f4{0.f, 0.f, 0.f, 0.f};
                    if (k < cnt && id >= 0 && act) x[u] = *reinterpret_cast<const f4*>(a.H + (size_t)id * a.D + col);
                }
#pragma unroll
                for (int u = 0; u < TW_UN; ++u)
                    if ((j0 + u) * G + grp < cnt) { s4.x += x[u].x; s4.y += x[u].y; s4.z += x[u].z; s4.w += x[u].w; }
            }
        } else {
            for (int j0 = 0; j0 < cnt; j0 += TW_UN) {
                float x[TW_UN][4];
#pragma unroll
                for (int u = 0; u < TW_UN; ++u) {
                    const int id = __shfl(mine, (j0 + u) & 63);
                    const bool live = j0 + u < cnt && id >= 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[u][e] = (live && lane + 64 * e < a.D) ? a.H[(size_t)id * a.D + lane + 64 * e] : 0.0f;
                }
#pragma unroll
                for (int u = 0; u < TW_UN; ++u)
                    if (j0 + u < cnt) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) s[e] += x[u][e];
                    }
            }
        }
    }
    if (LPR > 0) {
#pragma unroll
        for (int off = 32; off >= P; off >>= 1) {
            s4.x += __shfl_xor(s4.x, off); s4.y += __shfl_xor(s4.y, off); s4.z += __shfl_xor(s4.z, off); s4.w += __shfl_xor(s4.w, off);
        }
    }
    const bool dead = __ballot(bad) != 0ull;
    float c = 0.0f;
    if (!dead && sp.len > 0) c = a.mode == ORX_BAG_MEAN ? 1.0f / (float)sp.len : a.inv_denom;
    if (lane == 0) {
        if (dead) *a.err = 1;
        if (a.uid) a.uid[i] = dead ? -1 : (int32_t)i;
        if (a.coef) a.coef[i] = c;
    }
    float* row = t.x[0] + (size_t)i * t.ldx[0];
    int c0 = 0;
#pragma unroll
    for (int j = 0; j < ORX_TOWER_SIDE; ++j)
        if (j < t.m) {
            const float* sr = t.S[j] + (size_t)sid[j] * t.sd[j];
            for (int cc = lane; cc < t.sd[j]; cc += 64) {
                const float v = dead ? 0.0f : sr[cc];
                row[c0 + cc] = v;
            }
            c0 += t.sd[j];
        }
    float* pr = row + t.so;
    if (LPR > 0) {
        if (grp == 0 && act) {
            f4 q = {0.f, 0.f, 0.f, 0.f};
            if (c != 0.0f) q = f4{c * s4.x, c * s4.y, c * s4.z, c * s4.w};
            pr[col] = q.x; pr[col + 1] = q.y; pr[col + 2] = q.z; pr[col + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (lane + 64 * e < a.D) pr[lane + 64 * e] = c != 0.0f ? c * s[e] : 0.0f;
    }
    for (int cc = t.w[0] + lane; cc < t.ldx[0]; cc += 64) row[cc] = 0.0f;
}

// round(round(a b) + c): the l2 term as fs_finish_kernel's fmaf(scale, s, l2 x) rounds it at scale 1 -- the product once, then the sum
__device__ __forceinline__ float tw_l2_add(float a, float b, float c) {
#pragma clang fp contract(off)
    const float p = a * b;
    return c + p;
}

// rows [row0, row0 + 64) x columns [0, Wp) of X (stride ld, `width` true columns) into LDS [64][pitch], zeros beyond B and width
__device__ __forceinline__ void tw_tile(float* dst, int pitch, const float* X, int ld, int width, int Wp, int64_t row0, int64_t B, int tid) {
    for (int e = tid; e < 64 * Wp; e += 256) {
        const int r = e / Wp, k = e - r * Wp;
        const int64_t row = row0 + r;
        dst[r * pitch + k] = (row < B && k < width) ? X[(size_t)row * ld + k] : 0.0f;
    }
}

__global__ __launch_bounds__(256) void tower_forward_kernel(TowerArgs t, int l) {
    extern __shared__ __attribute__((aligned(16))) float tw_lds[];
    const int K = t.w[l], N = t.w[l + 1], Kp = (K + 15) & ~15, pitch = Kp + 4, nnb = (N + 15) >> 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, ln = lane & 15;
    const int64_t row0 = (int64_t)blockIdx.x * 64;
    const float* W = t.W[l];
    const float* cb = t.c[l];
    const bool relu = l + 1 < t.L || t.relu_last;
    tw_tile(tw_lds, pitch, t.x[l], t.ldx[l], K, Kp, row0, t.B, tid);
    __syncthreads();
    f32x4 acc[TW_NB];
#pragma unroll
    for (int nb = 0; nb < TW_NB; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    // A: x[row 16 wave + ln][k0 + q];  B: W[k0 + q][16 nb + ln]
    const float* xr = tw_lds + (16 * wave + ln) * pitch + q;
    // Kp is a multiple of 16: four k steps per trip, their loads of W in flight together before the first product
    for (int k0 = 0; k0 < Kp; k0 += 16) {
        float av[4], bv[4][TW_NB];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            av[u] = xr[k0 + 4 * u];
            const int k = k0 + 4 * u + q;
            const float* wr = W + (size_t)k * N + ln;
#pragma unroll
            for (int nb = 0; nb < TW_NB; ++nb) bv[u][nb] = (nb < nnb && k < K && 16 * nb + ln < N) ? wr[16 * nb] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int nb = 0; nb < TW_NB; ++nb)
                if (nb < nnb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u][nb], acc[nb], 0, 0, 0);
    }
    // acc[nb][r] = (row 16 wave + 4 q + r, column 16 nb + ln)
    float* Y = t.x[l + 1];
    const int ldy = t.ldx[l + 1];
#pragma unroll
    for (int nb = 0; nb < TW_NB; ++nb)
        if (nb < nnb) {
            const int n = 16 * nb + ln;
            if (n < N) {
                const float bias = cb ? cb[n] : 0.0f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t row = row0 + 16 * wave + 4 * q + r;
                    if (row < t.B) {
                        float v = acc[nb][r] + bias;
                        if (relu) v = v > 0.0f ? v : 0.0f;
                        Y[(size_t)row * ldy + n] = v;
                    }
                }
            }
        }
}

__global__ __launch_bounds__(256) void tower_backward_kernel(TowerArgs t, int l) {
    extern __shared__ __attribute__((aligned(16))) float tw_lds[];
    const int K = t.w[l], N = t.w[l + 1], Kp = (K + 15) & ~15, Np = (N + 15) & ~15, px = Kp + 4, pg = Np + 4;
    const int nkb = Kp >> 4, nnb = Np >> 4;
    float* Xs = tw_lds;                     // [64][px] x_l
    float* Gs = Xs + 64 * px;               // [64][pg] g_{l+1} .* mask
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, ln = lane & 15;
    const float* W = t.W[l];
    const bool relu = l + 1 < t.L || t.relu_last;
    const float* Y = t.x[l + 1];
    const int ldy = t.ldx[l + 1];
    const float* GY = t.g[l + 1];
    const int ldgy = t.ldg[l + 1];
    float* GX = t.g[l];
    const int ldgx = t.ldg[l];
    const float l2x = l == 0 ? t.l2x : 0.0f;
    const int chunk = blockIdx.x;
    const int64_t ntiles = (t.B + 63) >> 6;
    const int64_t t_beg = (int64_t)chunk * t.tpc, t_end = std::min<int64_t>(t_beg + t.tpc, ntiles);
    float* pw = t.pw[l] ? t.pw[l] + (size_t)chunk * K * N : nullptr;
    float* pc = t.pc[l] ? t.pc[l] + (size_t)chunk * N : nullptr;
    for (int64_t tile = t_beg; tile < t_end; ++tile) {
        const int64_t row0 = tile * 64;
        const bool first = tile == t_beg;
        tw_tile(Xs, px, t.x[l], t.ldx[l], K, Kp, row0, t.B, tid);
        for (int e = tid; e < 64 * Np; e += 256) {
            const int r = e / Np, n = e - r * Np;
            const int64_t row = row0 + r;
            float g = 0.0f;
            if (row < t.B && n < N) {
                g = GY[(size_t)row * ldgy + n];
                if (relu && !(Y[(size_t)row * ldy + n] > 0.0f)) g = 0.0f;
            }
            Gs[r * pg + n] = g;
        }
        __syncthreads();
        // dc: the tile's 64 rows in row order
        if (pc && tid < N) {
            float sum = 0.0f;
            for (int r = 0; r < 64; ++r) sum += Gs[r * pg + tid];
            pc[tid] = first ? sum : pc[tid] + sum;
        }
        // g_l [64][K] = gm [64][N] . W^T: A: gm[row 16 wave + ln][n0 + q];  B: W[16 kb + ln][n0 + q]
        if (GX) {
            f32x4 acc[TW_NB];
#pragma unroll
            for (int kb = 0; kb < TW_NB; ++kb) acc[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
            const float* gr = Gs + (16 * wave + ln) * pg + q;
            for (int n0 = 0; n0 < Np; n0 += 16) {       // (four n steps per trip, as the forward has its k steps)
                float av[4], bv[4][TW_NB];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    av[u] = gr[n0 + 4 * u];
                    const int n = n0 + 4 * u + q;
#pragma unroll
                    for (int kb = 0; kb < TW_NB; ++kb) {
                        const int k = 16 * kb + ln;
                        bv[u][kb] = (kb < nkb && k < K && n < N) ? W[(size_t)k * N + n] : 0.0f;
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int kb = 0; kb < TW_NB; ++kb)
                        if (kb < nkb) acc[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u][kb], acc[kb], 0, 0, 0);
            }
#pragma unroll
            for (int kb = 0; kb < TW_NB; ++kb)
                if (kb < nkb) {
                    const int k = 16 * kb + ln;
                    if (k < K) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int lr = 16 * wave + 4 * q + r;
                            const int64_t row = row0 + lr;
                            if (row < t.B) GX[(size_t)row * ldgx + k] = tw_l2_add(l2x, Xs[lr * px + k], acc[kb][r]);
                        }
                    }
                }
        }
        // dW [K][N] = x_l^T [K][64] . gm [64][N]: wavefront w owns the row blocks kb = w, w + 4, ..
        // A: x[row r0 + q][16 kb + ln];  B: gm[row r0 + q][16 nb + ln]
        if (pw) {
            for (int kb = wave; kb < nkb; kb += 4) {
                f32x4 acc[TW_NB];
#pragma unroll
                for (int nb = 0; nb < TW_NB; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
                for (int r0 = 0; r0 < 64; r0 += 4) {
                    const float av = Xs[(r0 + q) * px + 16 * kb + ln];
                    const float* gr = Gs + (r0 + q) * pg + ln;
#pragma unroll
                    for (int nb = 0; nb < TW_NB; ++nb)
                        if (nb < nnb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, gr[16 * nb], acc[nb], 0, 0, 0);
                }
#pragma unroll
                for (int nb = 0; nb < TW_NB; ++nb)
                    if (nb < nnb) {
                        const int n = 16 * nb + ln;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int k = 16 * kb + 4 * q + r;
                            if (k < K && n < N) {
                                float* p = pw + (size_t)k * N + n;
                                *p = first ? acc[nb][r] : *p + acc[nb][r];
                            }
                        }
                    }
            }
        }
        __syncthreads();                      // every wavefront is done with the tile
    }
}

// blockIdx.y: the layer; one thread per element of (W_l | c_l)
__global__ __launch_bounds__(256) void tower_finish_kernel(TowerArgs t) {
    const int l = blockIdx.y;
    const int K = t.w[l], N = t.w[l + 1];
    const int64_t KN = (int64_t)K * N;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < KN) {
        float s = 0.0f;
        for (int ch = 0; ch < t.nch; ++ch) s += t.pw[l][(size_t)ch * KN + idx];
        t.GW[l][idx] = fmaf(t.l2m, t.W[l][idx], s);
    } else if (idx < KN + N && t.c[l]) {
        const int n = (int)(idx - KN);
        float s = 0.0f;
        for (int ch = 0; ch < t.nch; ++ch) s += t.pc[l][(size_t)ch * N + n];
        t.Gc[l][n] = fmaf(t.l2m, t.c[l][n], s);
    }
}

inline int tw_lpr(const BagArgs& a) {        // 0: the plain walk (bag_lpr of kernels_bag.hip for an output on 16 bytes)
    if (a.D % 4 != 0 || a.D > 256 || (uintptr_t)a.H % 16 != 0) return 0;
    int lpr = 4;
    while (4 * lpr < a.D) lpr *= 2;
    return lpr;
}

}  // namespace

// at most 32 batch chunks: the partials of a 256 x 256 layer stay below 8 MB whatever B is
void orx_tower_plan(int64_t B, int* nch, int* tpc) {
    const int64_t ntiles = std::max<int64_t>(1, (B + 63) >> 6);
    const int64_t t = (ntiles + 31) / 32;
    *tpc = (int)t;
    *nch = (int)((ntiles + t - 1) / t);
}

int orx_launch_tower_input(orx_ctx* ctx, const TowerArgs& a) {
    if (a.B == 0) return ORX_OK;
    ProfScope ps(ctx, ORX_K_FUSED);
    const dim3 g((unsigned)((a.B + 3) / 4));
    switch (tw_lpr(a.bag)) {
        case 4: ORX_LAUNCH(ctx, tower_input_kernel<4>, g, dim3(256), 0, a); break;
        case 8: ORX_LAUNCH(ctx, tower_input_kernel<8>, g, dim3(256), 0, a); break;
        case 16: ORX_LAUNCH(ctx, tower_input_kernel<16>, g, dim3(256), 0, a); break;
        case 32: ORX_LAUNCH(ctx, tower_input_kernel<32>, g, dim3(256), 0, a); break;
        case 64: ORX_LAUNCH(ctx, tower_input_kernel<64>, g, dim3(256), 0, a); break;
        default: ORX_LAUNCH(ctx, tower_input_kernel<0>, g, dim3(256), 0, a); break;
    }
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

int orx_launch_tower_forward(orx_ctx* ctx, const TowerArgs& a) {
    if (a.B == 0) return ORX_OK;
    ORX_ONCE_PER_DEVICE(ctx, ORX_HIP(hipFuncSetAttribute((const void*)tower_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024)));
    for (int l = 0; l < a.L; ++l) {
        ProfScope ps(ctx, ORX_K_GEMM);
        const size_t lds = (size_t)64 * (((a.w[l] + 15) & ~15) + 4) * sizeof(float);
        ORX_LAUNCH(ctx, tower_forward_kernel, dim3((unsigned)((a.B + 63) >> 6)), dim3(256), lds, a, l);
        ORX_HIP(hipGetLastError());
    }
    return ORX_OK;
}

int orx_launch_tower_backward(orx_ctx* ctx, const TowerArgs& a) {
    if (a.B == 0) return ORX_OK;
    ORX_ONCE_PER_DEVICE(ctx, ORX_HIP(hipFuncSetAttribute((const void*)tower_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 136 * 1024)));
    for (int l = a.L - 1; l >= 0; --l) {
        if (!a.g[l] && !a.pw[l]) continue;            // nothing below this layer takes a gradient
        ProfScope ps(ctx, ORX_K_GEMM);
        const size_t lds = (size_t)64 * (((a.w[l] + 15) & ~15) + ((a.w[l + 1] + 15) & ~15) + 8) * sizeof(float);
        ORX_LAUNCH(ctx, tower_backward_kernel, dim3((unsigned)a.nch), dim3(256), lds, a, l);
        ORX_HIP(hipGetLastError());
    }
    return ORX_OK;
}

int orx_launch_tower_finish(orx_ctx* ctx, const TowerArgs& a) {
    int64_t most = 0;
    for (int l = 0; l < a.L; ++l) most = std::max<int64_t>(most, (int64_t)a.w[l] * a.w[l + 1] + a.w[l + 1]);
    ProfScope ps(ctx, ORX_K_FUSED);
    ORX_LAUNCH(ctx, tower_finish_kernel, dim3((unsigned)((most + 255) / 256), (unsigned)a.L), dim3(256), 0, a);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}
