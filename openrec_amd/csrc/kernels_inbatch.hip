// In-batch negatives (orx_inbatch_step / orx_inbatch_loss, include/openrec_hip.h has the semantics): the softmax of every sample's
// positive against the positives of the whole batch, s_ij = scale (u_i . v_j + b_j) + off_j, without a B x B matrix.
//
// Five kernels per step, none of which writes a table, so every gradient is taken on the pre-step tables:
//   inbatch_gather_kernel    U[uid] and V[pid] once into contiguous rows xu / xv [Bp][Dp] (Bp = B rounded up to 64, Dp = D rounded
//                            up to 16, zeros beyond B and D), and per sample: key (pid, -1 for a sample with an id out of range
//                            and for the padding), the bias, the offset, c = w / B and |u|^2 + |v|^2.  One wavefront per sample.
//   inbatch_walk_kernel<0>   the LSE pass.  A workgroup owns 64 rows i (wavefront w 16 of them, in LDS once) and walks the columns
//                            of its chunk in tiles of 64 gathered rows: v_mfma_f32_16x16x4_f32 in the layout of kernels_score.hip,
//                            the WALKED rows as the M side, so lane l ends up with S[walked 16 s + 4 (l / 16) + r][own l % 16].
//                            Every lane keeps (m, E_off, s_ii) of its own row over its share of the columns online; the four lane
//                            groups of a row merge in lane-group order at the end, the chunks in chunk order in
//   inbatch_finalize_kernel  m_i, c_i / tot_i (pi_ij = exp(s_ij - m_i) / tot_i: no log on the way to a gradient -- a logarithm that
//                            is one ulp off at lse = 7 tilts every pi of the row by 5e-7), the diagonal's coefficient -c_i A_i, l_i,
//                            and one (loss, l2) partial per workgroup, which
//                            loss_reduce_kernel adds in a fixed order.
//   inbatch_walk_kernel<1|2> the gradient pass of the user side (own rows i, walked columns j) and of the item side (own rows j,
//                            walked rows i: m, c / tot are then the walked side's, b and off the own side's).  The S tile is
//                            recomputed and turned into the coefficients a_ij IN the accumulator registers.  Because the walked
//                            rows were the M side, these registers already are the A operand of the second product: lane l holds
//                            a[own l % 16][walked 16 s + 4 (l / 16) + c], which is A[m = l % 16][k = l / 16] of step (s, c) when the
//                            k order inside a block of 16 walked rows is (lane group, c) -- the sum does not care.  The B operand
//                            is X[walked 16 s + 4 (l / 16) + c][16 kb + l % 16], one ds_read_b32 per step out of the same LDS tile
//                            (row pitch Dp + 4: the two lane groups of a 32-lane half sit 16 banks apart).  G[own 16][Dp] +=
//                            a[16][64] . X[64][Dp] with Dp / 16 independent accumulators per wavefront, interleaved.  The item
//                            side also sums its coefficients per own row: the bias gradient.
//   inbatch_finish_kernel    adds the chunks' partial G tiles in chunk order, scales, adds l2_reg x and writes the gradient rows
//                            [B][gs] that orx_apply_rows takes, the bias gradient in column D of the item side's.
// The next tile's rows are fetched into registers while the present one is multiplied and laid into the ONE tile buffer after it
// (two tile buffers of 64 x 260 floats beside the own rows do not fit the LDS at D = 256).
// Masking is a compare of keys: a column whose key is < 0 is in nobody's softmax; with mask_hits, neither is a column j != i with
// key[j] == key[i].  A row with key < 0 has c = 0, m = +inf (every exp(s - m) is 0) and a diagonal coefficient of 0.
// No atomics anywhere: every sum has a fixed order.
#include <algorithm>

#include "orx_device.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr float IB_NEG = -3.0e38f;            // "no column yet": finite, so that exp(m - m) of an empty share is 1, not NaN

// exp(x) for x <= ~0 to about one ulp of v_exp_f32.  __expf rounds x log2(e) to fp32 with a constant that is itself 1.3e-8 off: at
// x = -7 (a pi of 1 / 1100) every exp of a row leans the same way by 1.4e-7, the column sums of the pi with it, while A_i comes
// from exps of other arguments.  Here the product's rounding error and the constant's low part are put back to first order.
// Arguments below -104 (2^-150, and the -inf of a masked column) give 0.
__device__ __forceinline__ float ib_exp(float x) {
    x = fmaxf(x, -104.0f);
    const float hi = 1.44269502162933349609375f, lo = 1.92596299e-8f;
    const float t = x * hi;
    const float r = fmaf(x, lo, fmaf(x, hi, -t));
    const float e = __builtin_amdgcn_exp2f(t);
    return fmaf(e, r * 0.693147182f, e);
}

// s += x with the rounding error of the sum carried in c (Kahan).  A lane's running sums take one term per tile, all of one sign:
// added plainly, the B / 64 terms of a walk lose about sqrt(B / 64) ulp, which the bias gradient -- a difference of two such sums
// that cancels to a hundredth of either -- cannot afford
__device__ __forceinline__ void ib_add(float& s, float& c, float x) {
    const float y = x - c, t = s + y;
    c = (t - s) - y;
    s = t;
}

__global__ __launch_bounds__(256) void inbatch_gather_kernel(InBatchArgs a) {
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
    for (int c = lane; c < a.Dp; c += 64) {
        const bool in = ok && c < a.D;
        const float x = in ? ur[c] : 0.0f, y = in ? vr[c] : 0.0f;
        a.xu[(size_t)t * a.Dp + c] = x;
        a.xv[(size_t)t * a.Dp + c] = y;
        sq = fmaf(x, x, fmaf(y, y, sq));
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

// MODE 0: the LSE pass; 1: the gradients of the user side; 2: of the item side.  KBMAX: the power of two at or above Dp / 16
template <int MODE, int KBMAX>
__global__ __launch_bounds__(256) void inbatch_walk_kernel(InBatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ib_lds[];
    const int Dp = a.Dp, nkb = Dp >> 4, pitch = Dp + 4, q4 = Dp >> 2;
    float* As = ib_lds;                                     // [64][pitch] the own rows
    float* Bs = As + 64 * pitch;                            // [64][pitch] the tile of walked rows
    int* wkey = reinterpret_cast<int*>(Bs + 64 * pitch);    // [64] the tile's keys
    float* wa = reinterpret_cast<float*>(wkey + 64);        // [64] MODE 0 / 1: the tile's biases;  MODE 2: its c / tot
    float* wb = wa + 64;                                    // [64] MODE 0 / 1: the tile's offsets; MODE 2: its row maxima
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, ln = lane & 15;
    const float* Xo = MODE == 2 ? a.xv : a.xu;
    const float* Xw = MODE == 2 ? a.xu : a.xv;
    const int64_t o0 = (int64_t)blockIdx.x * 64;
    const int chunk = blockIdx.y;
    const int ntiles = (int)(a.Bp >> 6);
    const int t_beg = chunk * a.tpc;
    const int t_end = t_beg + a.tpc < ntiles ? t_beg + a.tpc : ntiles;
    {
        const f32x4* src = reinterpret_cast<const f32x4*>(Xo + (size_t)o0 * Dp);
        for (int e = tid; e < 64 * q4; e += 256) {
            const int r = e / q4, c = e - r * q4;
            *reinterpret_cast<f32x4*>(As + r * pitch + 4 * c) = src[e];
        }
    }
    f32x4 stage[KBMAX];
    int skey = 0;
    float sa = 0.0f, sb = 0.0f;
    auto fetch = [&](int tile) {
        const f32x4* src = reinterpret_cast<const f32x4*>(Xw + (size_t)tile * 64 * Dp);     // 64 q4 = 256 nkb float4, contiguous
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
                const int e = tid + 256 * k, r = e / q4, c = e - r * q4;
                *reinterpret_cast<f32x4*>(Bs + r * pitch + 4 * c) = stage[k];
            }
        if (tid < 64) { wkey[tid] = skey; wa[tid] = sa; wb[tid] = sb; }
    };
    // this lane's own row: 16 per wavefront, the same one in the four lane groups
    const int64_t o = o0 + 16 * wave + ln;
    const int okey = a.key[o];
    const float own_a = MODE == 1 ? a.cn[o] : (MODE == 2 ? a.cb[o] : 0.0f);       // user side: c_i / tot_i; item side: b_j
    const float own_b = MODE == 1 ? a.rmax[o] : (MODE == 2 ? a.co[o] : 0.0f);     // user side: m_i;         item side: off_j
    const float dco = MODE == 0 ? 0.0f : a.dcoef[o];
    const float scale = a.scale;
    const bool mask = a.mask != 0;
    float m = IB_NEG, E = 0.0f, Ec = 0.0f, sd = -INFINITY;  // MODE 0
    float bsum = 0.0f, bc = 0.0f;                           // MODE 2
    f32x4 G[KBMAX];
#pragma unroll
    for (int k = 0; k < KBMAX; ++k) G[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* orow = As + (16 * wave + ln) * pitch + 4 * q;
    const float* wrow = Bs + ln * pitch + 4 * q;

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
                const f32x4 ov = *reinterpret_cast<const f32x4*>(orow + 16 * kb);
                f32x4 wv[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) wv[s] = *reinterpret_cast<const f32x4*>(wrow + s * 16 * pitch + 16 * kb);
                // four independent accumulators, interleaved: consecutive MFMAs never wait for each other's result
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[s][c], ov[c], acc[s], 0, 0, 0);
            }
        }
        // acc[s][r] = u . v of (walked row 64 tile + 16 s + 4 q + r, own row o)
        float tmax = IB_NEG, tsum = 0.0f;
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
                for (int r = 0; r < 4; ++r) {
                    const bool diag = (int64_t)tile * 64 + 16 * s + 4 * q + r == o;
                    e += diag ? 0.0f : ib_exp(acc[s][r] - mn);
                }
            const float f = ib_exp(m - mn);
            E *= f; Ec *= f;
            ib_add(E, Ec, e);
            m = mn;
        } else {
            if (MODE == 2) ib_add(bsum, bc, tsum);
            // G[own 16][Dp] += a[own 16][64 walked] . X[64 walked][Dp]: the coefficients are the A operand as they sit
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float* xr = Bs + (16 * s + 4 * q + c) * pitch + ln;
#pragma unroll
                    for (int kb = 0; kb < KBMAX; ++kb)
                        if (kb < nkb) G[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(acc[s][c], xr[16 * kb], G[kb], 0, 0, 0);
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
        float* gp = (MODE == 2 ? a.gpv : a.gpu) + (prow + (size_t)o0 + 16 * wave + 4 * q) * Dp + ln;
#pragma unroll
        for (int kb = 0; kb < KBMAX; ++kb)
            if (kb < nkb) {
#pragma unroll
                for (int r = 0; r < 4; ++r) gp[(size_t)r * Dp + 16 * kb] = G[kb][r];
            }
        if (MODE == 2) {
            bsum += __shfl_xor(bsum, 16);
            bsum += __shfl_xor(bsum, 32);
            if (q == 0) a.bpart[prow + o] = bsum;
        }
    }
}

// one thread per sample: the chunks' (m, E_off, s_ii) in chunk order -> m_i, c_i / tot_i, the diagonal's coefficient, l_i; one (loss, l2)
// partial per workgroup
__global__ __launch_bounds__(256) void inbatch_finalize_kernel(InBatchArgs a) {
    __shared__ float s_l[4], s_q[4];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float cl = 0.0f, sq = 0.0f;
    if (i < a.Bp) {
        float l = 0.0f, rmax = INFINITY, cn = 0.0f, dco = 0.0f;
        if (a.key[i] >= 0) {
            float M = IB_NEG, sd = -INFINITY;
            for (int ch = 0; ch < a.nch; ++ch) { M = fmaxf(M, a.pm[(size_t)ch * a.Bp + i]); sd = fmaxf(sd, a.psd[(size_t)ch * a.Bp + i]); }
            float E = 0.0f;
            for (int ch = 0; ch < a.nch; ++ch) E = fmaf(a.pe[(size_t)ch * a.Bp + i], ib_exp(a.pm[(size_t)ch * a.Bp + i] - M), E);
            const float tot = ib_exp(sd - M) + E;                  // (the diagonal's term is exactly 1 when it holds the maximum)
            l = sd == M ? log1pf(E) : (M - sd) + logf(tot);
            const float c = a.cw[i];
            rmax = M;
            cn = c / tot;
            dco = -cn * E;                                         // -c_i A_i: the off-diagonal pi themselves, never 1 - pi_ii
            cl = c * l;
            sq = a.sq[i];
        }
        a.rmax[i] = rmax; a.cn[i] = cn; a.dcoef[i] = dco; a.rowloss[i] = l;
    }
    cl = wave_sum(cl); sq = wave_sum(sq);
    if ((threadIdx.x & 63) == 0) { s_l[threadIdx.x >> 6] = cl; s_q[threadIdx.x >> 6] = sq; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float2 v;
        v.x = ((s_l[0] + s_l[1]) + s_l[2]) + s_l[3];
        v.y = 0.5f * (((s_q[0] + s_q[1]) + s_q[2]) + s_q[3]);
        *reinterpret_cast<float2*>(a.partial + 2 * (size_t)blockIdx.x) = v;
    }
}

// one thread per element of a gradient row pair: the chunks in chunk order, the scale, the l2 term
__global__ __launch_bounds__(256) void inbatch_finish_kernel(InBatchArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.B * a.gs) return;
    const int64_t o = idx / a.gs;
    const int d = (int)(idx - o * a.gs);
    float gu = 0.0f, gv = 0.0f;
    if (d < a.D) {
        float su = 0.0f, sv = 0.0f;
        for (int ch = 0; ch < a.nch; ++ch) {
            su += a.gpu[((size_t)ch * a.Bp + o) * a.Dp + d];
            sv += a.gpv[((size_t)ch * a.Bp + o) * a.Dp + d];
        }
        gu = fmaf(a.scale, su, a.l2w * a.xu[(size_t)o * a.Dp + d]);
        gv = fmaf(a.scale, sv, a.l2w * a.xv[(size_t)o * a.Dp + d]);
    } else if (d == a.D) {
        float sbias = 0.0f;
        for (int ch = 0; ch < a.nch; ++ch) sbias += a.bpart[(size_t)ch * a.Bp + o];
        gv = a.scale * sbias;
    }
    a.gu[idx] = gu;
    a.gi[idx] = gv;
}

template <int MODE>
int ib_walk(orx_ctx* ctx, const InBatchArgs& a) {
    const dim3 g((unsigned)(a.Bp >> 6), (unsigned)a.nch);
    const size_t lds = ((size_t)128 * (a.Dp + 4) + 192) * sizeof(float);
    int kbmax = 1;
    while (16 * kbmax < a.Dp) kbmax *= 2;
#define ORX_IB(KB) do { \
        ORX_ONCE_PER_DEVICE(ctx, ORX_HIP(hipFuncSetAttribute((const void*)inbatch_walk_kernel<MODE, KB>, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024))); \
        ORX_LAUNCH(ctx, (inbatch_walk_kernel<MODE, KB>), g, dim3(256), lds, a); } while (0)
    switch (kbmax) {
        case 1: ORX_IB(1); break;
        case 2: ORX_IB(2); break;
        case 4: ORX_IB(4); break;
        case 8: ORX_IB(8); break;
        default: ORX_IB(16); break;
    }
#undef ORX_IB
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

}  // namespace

// what the launcher does for (B, D): own rows per workgroup, columns per tile, column chunks per row block, padded dim.  The
// launcher's own chunking aims at 512 workgroups per walk and keeps at least four tiles per chunk; it depends on B alone.
void orx_inbatch_plan(int64_t B, int32_t D, int32_t chunk_cols, int32_t out[4], int* tiles_per_chunk) {
    const int64_t ntiles = (B + 63) / 64;
    int64_t tpc;
    if (chunk_cols > 0) tpc = chunk_cols / 64;
    else {
        const int64_t want = std::max<int64_t>(1, 512 / std::max<int64_t>(ntiles, 1));
        tpc = std::max<int64_t>(4, (ntiles + want - 1) / want);
    }
    tpc = std::max<int64_t>(1, std::min<int64_t>(tpc, std::max<int64_t>(ntiles, 1)));
    out[0] = 64; out[1] = 64;
    out[2] = (int32_t)std::max<int64_t>(1, (ntiles + tpc - 1) / tpc);
    out[3] = (D + 15) & ~15;
    if (tiles_per_chunk) *tiles_per_chunk = (int)tpc;
}

int orx_launch_inbatch_forward(orx_ctx* ctx, const InBatchArgs& a) {
    {
        ProfScope ps(ctx, ORX_K_FUSED);
        ORX_LAUNCH(ctx, inbatch_gather_kernel, dim3((unsigned)((a.Bp + 3) / 4)), dim3(256), 0, a);
        ORX_HIP(hipGetLastError());
    }
    {
        ProfScope ps(ctx, ORX_K_GEMM);
        CHECK(ib_walk<0>(ctx, a));
    }
    ProfScope ps(ctx, ORX_K_FUSED);
    ORX_LAUNCH(ctx, inbatch_finalize_kernel, dim3((unsigned)orx_inbatch_npartials(a.B)), dim3(256), 0, a);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

int orx_launch_inbatch_grads(orx_ctx* ctx, const InBatchArgs& a) {
    {
        ProfScope ps(ctx, ORX_K_GEMM);
        CHECK(ib_walk<1>(ctx, a));
    }
    {
        ProfScope ps(ctx, ORX_K_GEMM);
        CHECK(ib_walk<2>(ctx, a));
    }
    ProfScope ps(ctx, ORX_K_FUSED);
    ORX_LAUNCH(ctx, inbatch_finish_kernel, dim3((unsigned)((a.B * a.gs + 255) / 256)), dim3(256), 0, a);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}
