// The full softmax over all items (orx_fullsoftmax_step / orx_seqrec_full_step and their forwards, include/openrec_hip.h has the
// semantics): every sample's label against EVERY row of the item table, s_ij = scale (u_i . V[j] + b[j]) + off[j], without a
// B x NI matrix.  The walk is kernels_inbatch.hip's made rectangular and restated here: the same
// v_mfma_f32_16x16x4_f32 tile walk -- exact fp32, an fmaf chain --, the same exp, the same Kahan running sums, no logarithm on
// the way to a gradient.
//
// Seven kernels per step, none of which writes a table, so every gradient is taken on the pre-step tables:
//   fs_prepare_kernel        the query rows Q[qid] (the user table's rows, or the pooled rows of the SeqRec form with qid[i] = i)
//                            once into xq [Bp][Dp] (Bp = B rounded up to 64, Dp = D rounded up to 16, zeros beyond B and D), and
//                            per sample: key (pid, -1 for a sample with an id out of range and for the padding), c = w / B and
//                            |u|^2 + |V[pid]|^2.  One wavefront per sample.
//   fs_items_kernel          a zero-padded copy xv [NIp][Dp] of the item table (NIp = NI rounded up to 64), made once per step, and
//                            per item the bias and the offset (0 beyond NI): every tile fetch of the walks is an aligned float4 for
//                            any D <= 256.  An item's key is its row number, -1 beyond NI: the walks compute it.
//   fs_walk_kernel<0>        the LSE pass.  A workgroup owns 64 samples (wavefront w 16 of them, in LDS once) and walks the item
//                            tiles of its item chunk; the WALKED rows are the M side of the product, so lane l ends up with
//                            S[walked 16 s + 4 (l / 16) + r][own l % 16].  Every lane keeps (m, E_off, s_label) of its own row over
//                            its share of the items online -- the label is the walked item whose key is the own row's --; the four
//                            lane groups of a row merge in lane-group order at the end, the item chunks in chunk order in
//   fs_finalize_kernel       m_i, c_i / tot_i, the label's coefficient -c_i A_i, l_i, and one (loss, l2) partial per workgroup.
//   fs_walk_kernel<1>        the gradient of the query rows: own rows i, walked items j; the S tile is recomputed and turned into
//                            the coefficients a_ij IN the accumulator registers, which then are the A operand of
//                            G[own 16][Dp] += a[16][64] . X[64][Dp].  Partial tiles per item chunk.
//   fs_walk_kernel<2>        the gradient of the item side: own rows are 64 ITEMS per workgroup, walked rows the sample tiles of one
//                            sample chunk (m, c / tot and the label's coefficient are then the walked side's, b and off the own
//                            side's); the label test is walked key == own item.  It also sums the coefficients per own row (the
//                            bias gradient) and counts n_j, the live samples whose label the own item is.
//   fs_finish_kernel<0|1>    adds the chunks' partials in chunk order, scales, adds the l2 terms and writes g_u [B][gs] (the stride
//                            orx_apply_rows takes), G_V [NI][D] and G_b [NI] (contiguous, for the dense rule).
// A row with key < 0 has c = 0, m = +inf (every exp(s - m) is 0) and a label coefficient of 0.  An item with off = -inf has
// s = -inf in every row: its pi are exactly 0.  No atomics anywhere: every sum has a fixed order.
#include <algorithm>

#include "orx_device.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr float FS_NEG = -3.0e38f;            // "no column yet": finite, so that exp(m - m) of an empty share is 1, not NaN

// exp(x) for x <= ~0 to about one ulp of v_exp_f32 (kernels_inbatch.hip ib_exp, restated: the rounding error of x log2(e) and
// the constant's low part are put back to first order).  Arguments below -104 (2^-150, and the -inf of a removed item) give 0.
__device__ __forceinline__ float fs_exp(float x) {
    x = fmaxf(x, -104.0f);
    const float hi = 1.44269502162933349609375f, lo = 1.92596299e-8f;
    const float t = x * hi;
    const float r = fmaf(x, lo, fmaf(x, hi, -t));
    const float e = __builtin_amdgcn_exp2f(t);
    return fmaf(e, r * 0.693147182f, e);
}

// s += x with the rounding error of the sum carried in c (Kahan): a lane's running sums take one term per tile, all of one sign
__device__ __forceinline__ void fs_add(float& s, float& c, float x) {
    const float y = x - c, t = s + y;
    c = (t - s) - y;
    s = t;
}

__global__ __launch_bounds__(256) void fs_prepare_kernel(FullSoftmaxArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= a.Bp) return;
    const bool live = t < a.B;
    const int u = live ? a.qid[t] : 0, p = live ? a.pid[t] : 0;
    const bool ok = live && id_ok(u, a.NQ) && id_ok(p, a.NI);
    if (live && !ok && lane == 0) *a.err = 1;
    const float* ur = a.Q + (size_t)(ok ? u : 0) * a.D;
    const float* vr = a.V + (size_t)(ok ? p : 0) * a.D;
    float sq = 0.0f;
    const int cend = a.X0 && a.x0w > a.Dp ? a.x0w : a.Dp;
    for (int c = lane; c < cend; c += 64) {
        const bool in = ok && c < a.D;
        const float x = in ? ur[c] : 0.0f, y = in ? vr[c] : 0.0f;
        if (c < a.Dp) a.xq[(size_t)t * a.Dp + c] = x;
        // (X0: the rows whose squares are the query side's l2 term, in the place of the query's own)
        const float xs = a.X0 ? ((ok && c < a.x0w) ? a.X0[(size_t)t * a.x0ld + c] : 0.0f) : x;
        sq = fmaf(xs, xs, fmaf(y, y, sq));
    }
    sq = wave_sum(sq);
    if (lane == 0) {
        a.key[t] = ok ? p : -1;
        a.cw[t] = ok ? (a.wt ? a.wt[t] : 1.0f) * a.invB : 0.0f;
        a.sq[t] = sq;
    }
}

// one thread per element of the padded copy
__global__ __launch_bounds__(256) void fs_items_kernel(FullSoftmaxArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.NIp * a.Dp) return;
    const int64_t j = idx / a.Dp;
    const int c = (int)(idx - j * a.Dp);
    const bool in = j < a.NI;
    a.xv[idx] = (in && c < a.D) ? a.V[(size_t)j * a.D + c] : 0.0f;
    if (c == 0) {
        a.ib[j] = (in && a.b) ? a.b[j] : 0.0f;
        a.io[j] = (in && a.off) ? a.off[j] : 0.0f;
    }
}

// MODE 0: the LSE pass; 1: the gradient of the query rows; 2: of the item side.  KBMAX: the power of two at or above Dp / 16
template <int MODE, int KBMAX>
__global__ __launch_bounds__(256) void fs_walk_kernel(FullSoftmaxArgs a) {
    extern __shared__ __attribute__((aligned(16))) float fs_lds[];
    const int Dp = a.Dp, nkb = Dp >> 4, pitch = Dp + 4, q4 = Dp >> 2;
    float* As = fs_lds;                                     // [64][pitch] the own rows
    float* Bs = As + 64 * pitch;                            // [64][pitch] the tile of walked rows
    int* wkey = reinterpret_cast<int*>(Bs + 64 * pitch);    // [64] the tile's keys
    float* wa = reinterpret_cast<float*>(wkey + 64);        // [64] MODE 0 / 1: the tile's biases;  MODE 2: its c / tot
    float* wb = wa + 64;                                    // [64] MODE 0 / 1: the tile's offsets; MODE 2: its row maxima
    float* wd = wb + 64;                                    // [64] MODE 2: the tile's label coefficients
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, ln = lane & 15;
    const float* Xo = MODE == 2 ? a.xv : a.xq;
    const float* Xw = MODE == 2 ? a.xq : a.xv;
    const int64_t o0 = (int64_t)blockIdx.x * 64;
    const int chunk = blockIdx.y;
    const int ntiles = (int)((MODE == 2 ? a.Bp : a.NIp) >> 6);
    const int tpc = MODE == 2 ? a.tps : a.tpi;
    const int t_beg = chunk * tpc;
    const int t_end = t_beg + tpc < ntiles ? t_beg + tpc : ntiles;
    {
        const f32x4* src = reinterpret_cast<const f32x4*>(Xo + (size_t)o0 * Dp);
        for (int e = tid; e < 64 * q4; e += 256) {
            const int r = e / q4, c = e - r * q4;
            *reinterpret_cast<f32x4*>(As + r * pitch + 4 * c) = src[e];
        }
    }
    f32x4 stage[KBMAX];
    int skey = 0;
    float sa = 0.0f, sb = 0.0f, sd4 = 0.0f;
    auto fetch = [&](int tile) {
        const f32x4* src = reinterpret_cast<const f32x4*>(Xw + (size_t)tile * 64 * Dp);     // 64 q4 = 256 nkb float4, contiguous
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
                const int e = tid + 256 * k, r = e / q4, c = e - r * q4;
                *reinterpret_cast<f32x4*>(Bs + r * pitch + 4 * c) = stage[k];
            }
        if (tid < 64) { wkey[tid] = skey; wa[tid] = sa; wb[tid] = sb; if (MODE == 2) wd[tid] = sd4; }
    };
    // this lane's own row: 16 per wavefront, the same one in the four lane groups
    const int64_t o = o0 + 16 * wave + ln;
    const int okey = MODE == 2 ? (o < a.NI ? (int)o : -1) : a.key[o];
    const float own_a = MODE == 1 ? a.cn[o] : (MODE == 2 ? a.ib[o] : 0.0f);       // query side: c_i / tot_i; item side: b_j
    const float own_b = MODE == 1 ? a.rmax[o] : (MODE == 2 ? a.io[o] : 0.0f);     // query side: m_i;         item side: off_j
    const float dco = MODE == 1 ? a.dcoef[o] : 0.0f;
    const float scale = a.scale;
    float m = FS_NEG, E = 0.0f, Ec = 0.0f, sd = -INFINITY;  // MODE 0
    float bsum = 0.0f, bc = 0.0f;                           // MODE 2
    int nlab = 0;                                           // MODE 2
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
            if (MODE == 2) fs_add(bsum, bc, tsum);
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
        float* gp = (MODE == 2 ? a.gpv : a.gpq) + (prow + (size_t)o0 + 16 * wave + 4 * q) * Dp + ln;
#pragma unroll
        for (int kb = 0; kb < KBMAX; ++kb)
            if (kb < nkb) {
#pragma unroll
                for (int r = 0; r < 4; ++r) gp[(size_t)r * Dp + 16 * kb] = G[kb][r];
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

// one thread per sample: the item chunks' (m, E_off, s_label) in chunk order -> m_i, c_i / tot_i, the label's coefficient, l_i; one
// (loss, l2) partial per workgroup
__global__ __launch_bounds__(256) void fs_finalize_kernel(FullSoftmaxArgs a) {
    __shared__ float s_l[4], s_q[4];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float cl = 0.0f, sq = 0.0f;
    if (i < a.Bp) {
        float l = 0.0f, rmax = INFINITY, cn = 0.0f, dco = 0.0f;
        if (a.key[i] >= 0) {
            float M = FS_NEG, sd = -INFINITY;
            for (int ch = 0; ch < a.nci; ++ch) { M = fmaxf(M, a.pm[(size_t)ch * a.Bp + i]); sd = fmaxf(sd, a.psd[(size_t)ch * a.Bp + i]); }
            float E = 0.0f;
            for (int ch = 0; ch < a.nci; ++ch) E = fmaf(a.pe[(size_t)ch * a.Bp + i], fs_exp(a.pm[(size_t)ch * a.Bp + i] - M), E);
            const float tot = fs_exp(sd - M) + E;                  // (the label's term is exactly 1 when it holds the maximum)
            l = sd == M ? log1pf(E) : (M - sd) + logf(tot);
            const float c = a.cw[i];
            rmax = M;
            cn = c / tot;
            dco = -cn * E;                                         // -c_i A_i: the other items' pi themselves, never 1 - pi_label
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

// one thread per element: the chunks in chunk order, the scale, the l2 term.  SIDE 0: g_u [B][gs]; 1: G_V [NI][D] and G_b [NI]
template <int SIDE>
__global__ __launch_bounds__(256) void fs_finish_kernel(FullSoftmaxArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (SIDE == 0) {
        if (idx >= a.B * a.gs) return;
        const int64_t o = idx / a.gs;
        const int d = (int)(idx - o * a.gs);
        float g = 0.0f;
        if (d < a.D) {
            float s = 0.0f;
            for (int ch = 0; ch < a.nci; ++ch) s += a.gpq[((size_t)ch * a.Bp + o) * a.Dp + d];
            g = fmaf(a.scale, s, a.l2q * a.xq[(size_t)o * a.Dp + d]);
        }
        a.gu[idx] = g;
    } else {
        const int w = a.D + 1;
        if (idx >= a.NI * w) return;
        const int64_t j = idx / w;
        const int d = (int)(idx - j * w);
        if (d < a.D) {
            float s = 0.0f;
            int n = 0;
            for (int ch = 0; ch < a.ncs; ++ch) {
                s += a.gpv[((size_t)ch * a.NIp + j) * a.Dp + d];
                n += a.npart[(size_t)ch * a.NIp + j];
            }
            a.GV[(size_t)j * a.D + d] = fmaf(a.scale, s, (a.l2w * (float)n) * a.xv[(size_t)j * a.Dp + d]);
        } else {
            float s = 0.0f;
            for (int ch = 0; ch < a.ncs; ++ch) s += a.bpart[(size_t)ch * a.NIp + j];
            a.Gb[j] = a.scale * s;
        }
    }
}

template <int MODE>
int fs_walk(orx_ctx* ctx, const FullSoftmaxArgs& a) {
    const dim3 g((unsigned)((MODE == 2 ? a.NIp : a.Bp) >> 6), (unsigned)(MODE == 2 ? a.ncs : a.nci));
    const size_t lds = ((size_t)128 * (a.Dp + 4) + 256) * sizeof(float);
    int kbmax = 1;
    while (16 * kbmax < a.Dp) kbmax *= 2;
#define ORX_FS(KB) do { \
        ORX_ONCE_PER_DEVICE(ctx, ORX_HIP(hipFuncSetAttribute((const void*)fs_walk_kernel<MODE, KB>, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024))); \
        ORX_LAUNCH(ctx, (fs_walk_kernel<MODE, KB>), g, dim3(256), lds, a); } while (0)
    switch (kbmax) {
        case 1: ORX_FS(1); break;
        case 2: ORX_FS(2); break;
        case 4: ORX_FS(4); break;
        case 8: ORX_FS(8); break;
        default: ORX_FS(16); break;
    }
#undef ORX_FS
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

}  // namespace

// What the launcher does for (B, NI, D).  Its own chunking aims at 512 workgroups per walk and keeps at least four tiles per
// chunk: the item axis is cut for the sample-owning walks by B alone, the sample axis for the item-owning walk by NI alone -- more
// than one sample chunk only below 512 item blocks, so the item-side partials never pass 512 x 64 rows of Dp floats.
void orx_fullsoftmax_plan(int64_t B, int64_t NI, int32_t D, int32_t chunk_items, int32_t chunk_samples, FullSoftmaxPlan* p) {
    auto cut = [](int64_t ntiles, int64_t nblocks, int32_t forced, int64_t* tpc, int64_t* nch) {
        int64_t t;
        if (forced > 0) t = forced / 64;
        else {
            const int64_t want = std::max<int64_t>(1, 512 / std::max<int64_t>(nblocks, 1));
            t = std::max<int64_t>(4, (ntiles + want - 1) / want);
        }
        t = std::max<int64_t>(1, std::min<int64_t>(t, std::max<int64_t>(ntiles, 1)));
        *tpc = t;
        *nch = std::max<int64_t>(1, (ntiles + t - 1) / t);
    };
    p->Bp = (B + 63) & ~(int64_t)63;
    p->NIp = (NI + 63) & ~(int64_t)63;
    p->Dp = (D + 15) & ~15;
    cut(p->NIp >> 6, p->Bp >> 6, chunk_items, &p->tpi, &p->nci);
    cut(p->Bp >> 6, p->NIp >> 6, chunk_samples, &p->tps, &p->ncs);
}

// the item copy and the LSE pass: what the forward does between its prepare and its finalize (the label-set form,
// kernels_labelsets.hip, has a prepare and a finalize of its own around the same two launches)
int orx_launch_fullsoftmax_lse(orx_ctx* ctx, const FullSoftmaxArgs& a) {
    {
        ProfScope ps(ctx, ORX_K_FUSED);
        ORX_LAUNCH(ctx, fs_items_kernel, dim3((unsigned)((a.NIp * a.Dp + 255) / 256)), dim3(256), 0, a);
        ORX_HIP(hipGetLastError());
    }
    ProfScope ps(ctx, ORX_K_GEMM);
    return fs_walk<0>(ctx, a);
}

int orx_launch_fullsoftmax_forward(orx_ctx* ctx, const FullSoftmaxArgs& a) {
    {
        ProfScope ps(ctx, ORX_K_FUSED);
        ORX_LAUNCH(ctx, fs_prepare_kernel, dim3((unsigned)((a.Bp + 3) / 4)), dim3(256), 0, a);
        ORX_HIP(hipGetLastError());
    }
    CHECK(orx_launch_fullsoftmax_lse(ctx, a));
    ProfScope ps(ctx, ORX_K_FUSED);
    ORX_LAUNCH(ctx, fs_finalize_kernel, dim3((unsigned)orx_fullsoftmax_npartials(a.B)), dim3(256), 0, a);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

int orx_launch_fullsoftmax_grads(orx_ctx* ctx, const FullSoftmaxArgs& a, bool query_side, bool item_side) {
    if (query_side) {
        {
            ProfScope ps(ctx, ORX_K_GEMM);
            CHECK(fs_walk<1>(ctx, a));
        }
        ProfScope ps(ctx, ORX_K_FUSED);
        ORX_LAUNCH(ctx, fs_finish_kernel<0>, dim3((unsigned)((a.B * a.gs + 255) / 256)), dim3(256), 0, a);
        ORX_HIP(hipGetLastError());
    }
    if (item_side) {
        {
            ProfScope ps(ctx, ORX_K_GEMM);
            CHECK(fs_walk<2>(ctx, a));
        }
        ProfScope ps(ctx, ORX_K_FUSED);
        ORX_LAUNCH(ctx, fs_finish_kernel<1>, dim3((unsigned)((a.NI * (a.D + 1) + 255) / 256)), dim3(256), 0, a);
        ORX_HIP(hipGetLastError());
    }
    return ORX_OK;
}
