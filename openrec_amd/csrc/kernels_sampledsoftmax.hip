// Sampled softmax over a SHARED candidate list (orx_sampled_softmax_step / orx_seqrec_sampled_step and their forwards;
// include/openrec_hip.h has the semantics): every sample's label against one list of S candidate items,
// s_ic = scale (q_i . V[cand_c] + b[cand_c]) + off_c, in fp32 on v_mfma_f32_16x16x4_f32.  No B x S matrix is stored.
//
// Four kernels per step, none of which writes a table, so every gradient is taken on the pre-step tables:
//   ss_gather_kernel   one wavefront per row, one 16-byte load per lane: the S candidate rows into xc [Sp][Dp] (Sp = S rounded up
//                      to 64 and at least 64, Dp = D rounded up to 16, zeros beyond S and D) with their bias, offset and key (the
//                      item id; -1 for an id out of range, an offset of -inf and the padding), and the B query rows and label
//                      rows into xq / xp [Bp][Dp] with the label's key, bias and offset, c_i = w_i / B and |q|^2 + |v|^2.  It
//                      also writes the item side's row list [B + S]: the labels, then the candidates, -1 for a dropped entry.
//   ss_row_kernel      forward and query gradient in ONE launch.  A workgroup owns 64 query rows, wavefront w 16 of them, and
//                      keeps them in REGISTERS as the B operand of the score product for the whole kernel (Dp / 4 registers a
//                      lane: lane l holds q[own l % 16][16 kb + 4 (l / 16) + c]).  s_i+ comes from xp with two shuffles, no LDS.
//                      The workgroup then walks all Sp / 64 candidate tiles TWICE.  Walk 1: the S tile in the layout of
//                      kernels_inbatch.hip (the walked rows as the M side: lane l ends up with S[walked 16 s + 4 (l / 16) + r]
//                      [own l % 16]), key and hit masking, online maximum and sum per lane.  Between the walks the four lane
//                      groups of a row merge in lane-group order and every lane knows m_i, c_i / tot_i, l_i and a_i+ of its own
//                      row: no partials, no finalize launch.  Walk 2: S again, turned into a_ic IN the accumulator registers,
//                      which then are the A operand of G[own 16][Dp] += a[16][64] . X[64][Dp]; the B operand of that product is
//                      read out of a TRANSPOSED copy of the tile, XT[d][walked], so that one ds_read_b128 serves four MFMAs
//                      (out of the row-major copy it is one ds_read_b32 each).  The next tile's rows are in flight in registers
//                      under the present tile's products.  LDS at D = 256: 64 x 260 + 256 x 68 floats = 133 KB of gfx950's 160.
//                      Row pitch Dp + 4 and 64 + 4: the 16 lanes of a lane group start 4 banks apart, so a b128 read of a group
//                      covers 64 distinct banks.  The epilogue writes g_q into gu, the label entries into rows [0, B) of gi,
//                      m_i and c_i / tot_i for the column kernel, l_i, and one (loss, l2) partial per workgroup.
//                      GRADS = false compiles walk 2 out: the forward-only call, and a step that does not train the query side.
//   ss_col_kernel      the candidates' gradient.  A workgroup owns 64 candidate columns (in registers, as above) and walks the
//                      query rows of its sample chunk in tiles of 64: a_ic from the stored m_i and c_i / tot_i, G_c += a . Q out
//                      of the transposed copy, the bias gradient as the Kahan sum of the coefficients.  B is split into sample
//                      chunks (a function of (B, S) alone) so that a short candidate list still fills the machine.
//   ss_finish_kernel   adds the chunks' partial tiles in chunk order, scales, and writes rows [B, B + S) of gi.
// Masking is a compare of keys: a column whose key is < 0 is in nobody's softmax; with mask, neither is a column whose key is the
// row's own label.  A dead row has c = 0 and m = +inf (every exp(s - m) is 0).  No atomics anywhere: every sum has a fixed order.
#include <algorithm>

#include "orx_device.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr float SS_NEG = -3.0e38f;            // "no column yet": finite, so that exp(m - m) of an empty share is 1, not NaN
constexpr int SS_TP = 68;                     // row pitch of the transposed tile: 64 walked rows + 4

// exp(x) for x <= ~0 to about one ulp of v_exp_f32 (kernels_inbatch.hip ib_exp has the reasoning); below -104, and for the -inf of
// a masked column, 0
__device__ __forceinline__ float ss_exp(float x) {
    x = fmaxf(x, -104.0f);
    const float hi = 1.44269502162933349609375f, lo = 1.92596299e-8f;
    const float t = x * hi;
    const float r = fmaf(x, lo, fmaf(x, hi, -t));
    const float e = __builtin_amdgcn_exp2f(t);
    return fmaf(e, r * 0.693147182f, e);
}

// s += x with the rounding error of the sum carried in c (Kahan): a lane's running sums take one term per tile, all of one sign
__device__ __forceinline__ void ss_add(float& s, float& c, float x) {
    const float y = x - c, t = s + y;
    c = (t - s) - y;
    s = t;
}

// columns [4 c4, 4 c4 + 4) of a table row of D floats, zeros beyond D; vec: the row is 16-byte aligned (D % 4 == 0)
__device__ __forceinline__ f32x4 ss_load4(const float* row, int c4, int D, bool vec) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row == nullptr) return v;
    if (vec) {
        if (4 * c4 < D) v = *reinterpret_cast<const f32x4*>(row + 4 * c4);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * c4 + j < D) v[j] = row[4 * c4 + j];
    }
    return v;
}

__global__ __launch_bounds__(256) void ss_gather_kernel(SampledSoftmaxArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int q4 = a.Dp >> 2;                                // <= 64: one float4 per lane
    const bool vec = (a.D & 3) == 0 && ((reinterpret_cast<uintptr_t>(a.Q) | reinterpret_cast<uintptr_t>(a.V)) & 15) == 0;
    if (t < a.Bp) {
        const bool live = t < a.B;
        const int u = live ? a.qid[t] : 0, p = live ? a.pid[t] : 0;
        const bool ok = live && id_ok(u, a.NQ) && id_ok(p, a.NI);
        if (live && !ok && lane == 0) *a.err = 1;
        const f32x4 x = ss_load4(ok ? a.Q + (size_t)u * a.D : nullptr, lane, a.D, vec);
        const f32x4 y = ss_load4(ok ? a.V + (size_t)p * a.D : nullptr, lane, a.D, vec);
        if (lane < q4) {
            *reinterpret_cast<f32x4*>(a.xq + (size_t)t * a.Dp + 4 * lane) = x;
            *reinterpret_cast<f32x4*>(a.xp + (size_t)t * a.Dp + 4 * lane) = y;
        }
        float sq = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) sq = fmaf(x[j], x[j], fmaf(y[j], y[j], sq));
        sq = wave_sum(sq);
        if (lane == 0) {
            a.key[t] = ok ? p : -1;
            a.pb[t] = (ok && a.b) ? a.b[p] : 0.0f;
            a.po[t] = (ok && a.poff) ? a.poff[t] : 0.0f;
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
    const f32x4 x = ss_load4(in ? a.V + (size_t)id * a.D : nullptr, lane, a.D, vec);
    if (lane < q4) *reinterpret_cast<f32x4*>(a.xc + (size_t)c * a.Dp + 4 * lane) = x;
    if (lane == 0) {
        a.ckey[c] = in ? id : -1;
        a.cb[c] = (in && a.b) ? a.b[id] : 0.0f;
        a.co[c] = in ? off : 0.0f;
        if (a.list && live) a.list[a.B + c] = in ? id : -1;
    }
}

// One tile of 64 walked rows on its way global -> registers -> LDS: the row-major copy Bs [64][Dp + 4] every product of scores
// reads, the transposed copy Ts [Dp][68] the gradient product reads, and three per-row words (a key and two floats)
template <int KBMAX>
struct SsTile {
    f32x4 stage[KBMAX];
    int skey; float sa, sb;
    __device__ __forceinline__ void fetch(const float* X, const int32_t* key, const float* fa, const float* fb, int64_t tile, int Dp, int tid) {
        const f32x4* src = reinterpret_cast<const f32x4*>(X + (size_t)tile * 64 * Dp);      // 64 Dp / 4 = 256 (Dp / 16) float4, contiguous
#pragma unroll
        for (int k = 0; k < KBMAX; ++k)
            if (16 * k < Dp) stage[k] = src[tid + 256 * k];
        if (tid < 64) { skey = key[tile * 64 + tid]; sa = fa[tile * 64 + tid]; sb = fb[tile * 64 + tid]; }
    }
    __device__ __forceinline__ void put(float* Bs, float* Ts, int* wkey, float* wa, float* wb, int Dp, int tid, bool transposed) {
        const int q4 = Dp >> 2, pitch = Dp + 4;
#pragma unroll
        for (int k = 0; k < KBMAX; ++k)
            if (16 * k < Dp) {
                const int e = tid + 256 * k, r = e / q4, c = e - r * q4;
                *reinterpret_cast<f32x4*>(Bs + r * pitch + 4 * c) = stage[k];
                if (transposed) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) Ts[(4 * c + j) * SS_TP + r] = stage[k][j];
                }
            }
        if (tid < 64) { wkey[tid] = skey; wa[tid] = sa; wb[tid] = sb; }
    }
};

// acc[s][r] = x . y of (walked row 16 s + 4 q + r of the tile in Bs, the lane's own row in ov)
template <int KBMAX>
__device__ __forceinline__ void ss_dots(const f32x4 (&ov)[KBMAX], const float* wrow, int pitch, int nkb, f32x4 (&acc)[4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < KBMAX; ++kb) {
        if (kb < nkb) {
            f32x4 wv[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) wv[s] = *reinterpret_cast<const f32x4*>(wrow + s * 16 * pitch + 16 * kb);
            // four independent accumulators, interleaved: consecutive MFMAs never wait for each other's result
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[s][c], ov[kb][c], acc[s], 0, 0, 0);
        }
    }
}

// G[own 16][Dp] += a[own 16][64 walked] . X[64 walked][Dp]: the coefficients in acc are the A operand as they sit (k = the lane
// group, walked row 16 s + 4 q + c at step (s, c)); the B operand X[16 s + 4 q + c][16 kb + ln], c = 0 .. 3, is ONE 16-byte read
// of the transposed tile.  Up to four accumulators G[kb] are interleaved.
template <int KBMAX>
__device__ __forceinline__ void ss_accum(const f32x4 (&acc)[4], const float* Ts, int q, int ln, int nkb, f32x4 (&G)[KBMAX]) {
    constexpr int GRP = KBMAX < 4 ? KBMAX : 4;
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int k0 = 0; k0 < KBMAX; k0 += GRP) {
            if (k0 < nkb) {
                f32x4 xt[GRP];
#pragma unroll
                for (int j = 0; j < GRP; ++j)
                    if (k0 + j < nkb) xt[j] = *reinterpret_cast<const f32x4*>(Ts + (16 * (k0 + j) + ln) * SS_TP + 16 * s + 4 * q);
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int j = 0; j < GRP; ++j)
                        if (k0 + j < nkb) G[k0 + j] = __builtin_amdgcn_mfma_f32_16x16x4f32(acc[s][c], xt[j][c], G[k0 + j], 0, 0, 0);
            }
        }
}

// LDS of the two walking kernels: Bs, [Ts], three words per walked row, one per own row
__host__ __device__ inline size_t ss_lds_floats(int Dp, bool transposed) { return (size_t)64 * (Dp + 4) + (transposed ? (size_t)Dp * SS_TP : 0) + 4 * 64; }

template <bool GRADS, int KBMAX>
__global__ __launch_bounds__(256) void ss_row_kernel(SampledSoftmaxArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ss_lds[];
    const int Dp = a.Dp, nkb = Dp >> 4, pitch = Dp + 4;
    float* Bs = ss_lds;                                     // [64][pitch] the candidate tile, row-major
    float* Ts = Bs + 64 * pitch;                            // [Dp][SS_TP] the same tile, transposed (GRADS)
    int* wkey = reinterpret_cast<int*>(Ts + (GRADS ? Dp * SS_TP : 0));      // [64] the tile's keys
    float* wa = reinterpret_cast<float*>(wkey + 64);        // [64] its biases
    float* wb = wa + 64;                                    // [64] its offsets
    float* ap = wb + 64;                                    // [64] a_i+ of the own rows (the epilogue)
    __shared__ float s_l[4], s_q[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, ln = lane & 15;
    const int64_t o0 = (int64_t)blockIdx.x * 64;
    const int64_t o = o0 + 16 * wave + ln;                  // this lane's own row: 16 per wavefront, the same one in the four lane groups
    const int ntiles = a.Sp >> 6;
    const float scale = a.scale;
    const bool mask = a.mask != 0;

    // the own rows, for the whole kernel; the label's score from xp
    f32x4 ov[KBMAX];
    float dp = 0.0f;
#pragma unroll
    for (int kb = 0; kb < KBMAX; ++kb) {
        ov[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (kb < nkb) {
            ov[kb] = *reinterpret_cast<const f32x4*>(a.xq + (size_t)o * Dp + 16 * kb + 4 * q);
            const f32x4 pv = *reinterpret_cast<const f32x4*>(a.xp + (size_t)o * Dp + 16 * kb + 4 * q);
#pragma unroll
            for (int c = 0; c < 4; ++c) dp = fmaf(ov[kb][c], pv[c], dp);
        }
    }
    dp += __shfl_xor(dp, 16);
    dp += __shfl_xor(dp, 32);
    const int okey = a.key[o];
    const float sp = fmaf(scale, dp + a.pb[o], a.po[o]);    // s_i+
    const float cw = a.cw[o];

    SsTile<KBMAX> st;
    const float* wrow = Bs + ln * pitch + 4 * q;
    float m = SS_NEG, E = 0.0f, Ec = 0.0f;                  // walk 1
    float rmax = INFINITY, cn = 0.0f, apos = 0.0f;          // between the walks
    f32x4 G[KBMAX];
#pragma unroll
    for (int k = 0; k < KBMAX; ++k) G[k] = f32x4{0.f, 0.f, 0.f, 0.f};

    st.fetch(a.xc, a.ckey, a.cb, a.co, 0, Dp, tid);
    st.put(Bs, Ts, wkey, wa, wb, Dp, tid, GRADS && ntiles == 1);
    __syncthreads();
#pragma unroll
    for (int pass = 0; pass < (GRADS ? 2 : 1); ++pass) {
        for (int tile = 0; tile < ntiles; ++tile) {
            // the tile after this one: the next of this walk, or the first of walk 2
            const bool wrap = tile + 1 == ntiles;
            const bool more = !wrap || (GRADS && pass == 0);
            if (more) st.fetch(a.xc, a.ckey, a.cb, a.co, wrap ? 0 : tile + 1, Dp, tid);
            f32x4 acc[4];
            ss_dots<KBMAX>(ov, wrow, pitch, nkb, acc);
            float tmax = SS_NEG;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int base = 16 * s + 4 * q;
                const i32x4 k4 = *reinterpret_cast<const i32x4*>(wkey + base);
                const f32x4 a4 = *reinterpret_cast<const f32x4*>(wa + base);
                const f32x4 b4 = *reinterpret_cast<const f32x4*>(wb + base);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool out = k4[r] < 0 || okey < 0 || (mask && k4[r] == okey);
                    const float sc = fmaf(scale, acc[s][r] + a4[r], b4[r]);
                    if (pass == 0) {
                        acc[s][r] = out ? -INFINITY : sc;
                        tmax = fmaxf(tmax, acc[s][r]);
                    } else {
                        acc[s][r] = out ? 0.0f : cn * ss_exp(sc - rmax);      // a_ic, where it sits
                    }
                }
            }
            if (pass == 0) {
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
                ss_accum<KBMAX>(acc, Ts, q, ln, nkb, G);
            }
            __syncthreads();                  // every wavefront is done with the tile
            if (more) st.put(Bs, Ts, wkey, wa, wb, Dp, tid, GRADS && (pass == 1 || wrap));
            __syncthreads();
        }
        if (pass == 0) {
            // the four lane groups of a row, in lane-group order; then the label's own term
            float M = SS_NEG, mk[4], Ek[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                mk[k] = __shfl(m, ln + 16 * k); Ek[k] = __shfl(E, ln + 16 * k);
                M = fmaxf(M, mk[k]);
            }
            float Es = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) Es = fmaf(Ek[k], ss_exp(mk[k] - M), Es);
            float l = 0.0f;
            if (okey >= 0) {
                const float M2 = fmaxf(M, sp);
                const float Eo = Es * ss_exp(M - M2);                  // the candidates' sum at the row maximum
                const float tot = ss_exp(sp - M2) + Eo;                // (the label's term is exactly 1 when it holds the maximum)
                l = sp == M2 ? log1pf(Eo) : (M2 - sp) + logf(tot);
                rmax = M2;
                cn = cw / tot;
                apos = -cn * Eo;                                       // -c_i sum_c pi_ic: the pi themselves, never 1 - pi_+
            }
            if (q == 0) { a.rmax[o] = rmax; a.cn[o] = cn; a.rowloss[o] = l; ap[16 * wave + ln] = apos; }
            const float cl = wave_sum(q == 0 ? cw * l : 0.0f), sq = wave_sum(q == 0 ? a.sq[o] : 0.0f);
            if (lane == 0) { s_l[wave] = cl; s_q[wave] = sq; }
            __syncthreads();
            if (tid == 0) {
                float2 v;
                v.x = ((s_l[0] + s_l[1]) + s_l[2]) + s_l[3];
                v.y = 0.5f * (((s_q[0] + s_q[1]) + s_q[2]) + s_q[3]);
                *reinterpret_cast<float2*>(a.partial + 2 * (size_t)blockIdx.x) = v;
            }
        }
    }

    // the epilogue.  G[kb][r] is (own row 16 wave + 4 q + r, column 16 kb + ln): g_q into gu, the label entry into row i of gi
    const int gs = a.gs, D = a.D;
    if (GRADS || a.gi) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int lr = 16 * wave + 4 * q + r;
            const int64_t row = o0 + lr;
            if (row >= a.B) continue;
            const float ar = ap[lr];
#pragma unroll
            for (int kb = 0; kb < KBMAX; ++kb) {
                const int d = 16 * kb + ln;
                if (kb < nkb && d < D) {
                    const float xq = a.xq[(size_t)row * Dp + d], xp = a.xp[(size_t)row * Dp + d];
                    if (GRADS) a.gu[(size_t)row * gs + d] = fmaf(scale, fmaf(ar, xp, G[kb][r]), a.l2w * xq);
                    if (a.gi) a.gi[(size_t)row * gs + d] = fmaf(scale * ar, xq, a.l2w * xp);
                }
            }
        }
        const int extra = gs - D;                           // the bias gradient in column D, zeros behind it
        for (int e = tid; e < 64 * extra; e += 256) {
            const int lr = e / extra, d = D + (e - lr * extra);
            const int64_t row = o0 + lr;
            if (row >= a.B) continue;
            if (GRADS) a.gu[(size_t)row * gs + d] = 0.0f;
            if (a.gi) a.gi[(size_t)row * gs + d] = d == D ? scale * ap[lr] : 0.0f;
        }
    }
}

template <int KBMAX>
__global__ __launch_bounds__(256) void ss_col_kernel(SampledSoftmaxArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ss_lds[];
    const int Dp = a.Dp, nkb = Dp >> 4, pitch = Dp + 4;
    float* Bs = ss_lds;                                     // [64][pitch] the tile of query rows, row-major
    float* Ts = Bs + 64 * pitch;                            // [Dp][SS_TP] the same tile, transposed
    int* wkey = reinterpret_cast<int*>(Ts + Dp * SS_TP);    // [64] the rows' label keys
    float* wa = reinterpret_cast<float*>(wkey + 64);        // [64] their c_i / tot_i
    float* wb = wa + 64;                                    // [64] their maxima m_i
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, ln = lane & 15;
    const int64_t o0 = (int64_t)blockIdx.x * 64;
    const int64_t o = o0 + 16 * wave + ln;                  // this lane's own candidate
    const int chunk = blockIdx.y;
    const int ntiles = (int)(a.Bp >> 6);
    const int t_beg = chunk * a.tps;
    const int t_end = t_beg + a.tps < ntiles ? t_beg + a.tps : ntiles;
    const float scale = a.scale;
    const bool mask = a.mask != 0;

    f32x4 ov[KBMAX];
#pragma unroll
    for (int kb = 0; kb < KBMAX; ++kb) {
        ov[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (kb < nkb) ov[kb] = *reinterpret_cast<const f32x4*>(a.xc + (size_t)o * Dp + 16 * kb + 4 * q);
    }
    const int okey = a.ckey[o];
    const float ob = a.cb[o], oo = a.co[o];

    SsTile<KBMAX> st;
    const float* wrow = Bs + ln * pitch + 4 * q;
    float bsum = 0.0f, bc = 0.0f;
    f32x4 G[KBMAX];
#pragma unroll
    for (int k = 0; k < KBMAX; ++k) G[k] = f32x4{0.f, 0.f, 0.f, 0.f};

    st.fetch(a.xq, a.key, a.cn, a.rmax, t_beg, Dp, tid);
    st.put(Bs, Ts, wkey, wa, wb, Dp, tid, true);
    __syncthreads();
    for (int tile = t_beg; tile < t_end; ++tile) {
        const bool more = tile + 1 < t_end;
        if (more) st.fetch(a.xq, a.key, a.cn, a.rmax, tile + 1, Dp, tid);
        f32x4 acc[4];
        ss_dots<KBMAX>(ov, wrow, pitch, nkb, acc);
        float tsum = 0.0f;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int base = 16 * s + 4 * q;
            const i32x4 k4 = *reinterpret_cast<const i32x4*>(wkey + base);
            const f32x4 a4 = *reinterpret_cast<const f32x4*>(wa + base);
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(wb + base);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool out = okey < 0 || k4[r] < 0 || (mask && k4[r] == okey);
                const float sc = fmaf(scale, acc[s][r] + ob, oo);
                const float co = out ? 0.0f : a4[r] * ss_exp(sc - b4[r]);
                acc[s][r] = co;
                tsum += co;
            }
        }
        ss_add(bsum, bc, tsum);
        ss_accum<KBMAX>(acc, Ts, q, ln, nkb, G);
        __syncthreads();                      // every wavefront is done with the tile
        if (more) st.put(Bs, Ts, wkey, wa, wb, Dp, tid, true);
        __syncthreads();
    }
    const size_t prow = (size_t)chunk * a.Sp;
    float* gp = a.gpc + (prow + (size_t)o0 + 16 * wave + 4 * q) * Dp + ln;
#pragma unroll
    for (int kb = 0; kb < KBMAX; ++kb)
        if (kb < nkb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) gp[(size_t)r * Dp + 16 * kb] = G[kb][r];
        }
    bsum += __shfl_xor(bsum, 16);
    bsum += __shfl_xor(bsum, 32);
    if (q == 0) a.bpc[prow + o] = bsum;
}

// one thread per element of a candidate's gradient row: the sample chunks in chunk order, the scale; no l2 on a candidate
__global__ __launch_bounds__(256) void ss_finish_kernel(SampledSoftmaxArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)a.S * a.gs) return;
    const int64_t c = idx / a.gs;
    const int d = (int)(idx - c * a.gs);
    float g = 0.0f;
    if (d < a.D) {
        for (int ch = 0; ch < a.ncs; ++ch) g += a.gpc[((size_t)ch * a.Sp + c) * a.Dp + d];
        g *= a.scale;
    } else if (d == a.D) {
        for (int ch = 0; ch < a.ncs; ++ch) g += a.bpc[(size_t)ch * a.Sp + c];
        g *= a.scale;
    }
    a.gi[(size_t)(a.B + c) * a.gs + d] = g;
}

int ss_kbmax(int Dp) {
    int kbmax = 1;
    while (16 * kbmax < Dp) kbmax *= 2;
    return kbmax;
}

template <bool GRADS>
int ss_rows(orx_ctx* ctx, const SampledSoftmaxArgs& a) {
    const dim3 g((unsigned)(a.Bp >> 6));
    const size_t lds = ss_lds_floats(a.Dp, GRADS) * sizeof(float);
#define ORX_SS(KB) do { \
        ORX_ONCE_PER_DEVICE(ctx, ORX_HIP(hipFuncSetAttribute((const void*)ss_row_kernel<GRADS, KB>, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024))); \
        ORX_LAUNCH(ctx, (ss_row_kernel<GRADS, KB>), g, dim3(256), lds, a); } while (0)
    switch (ss_kbmax(a.Dp)) {
        case 1: ORX_SS(1); break;
        case 2: ORX_SS(2); break;
        case 4: ORX_SS(4); break;
        case 8: ORX_SS(8); break;
        default: ORX_SS(16); break;
    }
#undef ORX_SS
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

int ss_cols(orx_ctx* ctx, const SampledSoftmaxArgs& a) {
    const dim3 g((unsigned)(a.Sp >> 6), (unsigned)a.ncs);
    const size_t lds = ss_lds_floats(a.Dp, true) * sizeof(float);
#define ORX_SS(KB) do { \
        ORX_ONCE_PER_DEVICE(ctx, ORX_HIP(hipFuncSetAttribute((const void*)ss_col_kernel<KB>, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024))); \
        ORX_LAUNCH(ctx, (ss_col_kernel<KB>), g, dim3(256), lds, a); } while (0)
    switch (ss_kbmax(a.Dp)) {
        case 1: ORX_SS(1); break;
        case 2: ORX_SS(2); break;
        case 4: ORX_SS(4); break;
        case 8: ORX_SS(8); break;
        default: ORX_SS(16); break;
    }
#undef ORX_SS
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

}  // namespace

// what the launchers do for (B, S, D): the padded sizes, and the sample chunks of the column kernel -- it aims at 512 workgroups
// and keeps at least four tiles per chunk; a function of (B, S) alone
void orx_sampledsoftmax_plan(int64_t B, int64_t S, int32_t D, SampledSoftmaxPlan* p) {
    p->Bp = (B + 63) & ~(int64_t)63;
    p->Sp = std::max<int64_t>(64, (S + 63) & ~(int64_t)63);
    p->Dp = (D + 15) & ~15;
    const int64_t ntiles = std::max<int64_t>(1, p->Bp >> 6);
    const int64_t want = std::max<int64_t>(1, 512 / (p->Sp >> 6));
    p->tps = std::min<int64_t>(ntiles, std::max<int64_t>(4, (ntiles + want - 1) / want));
    p->ncs = (ntiles + p->tps - 1) / p->tps;
}

int orx_launch_sampledsoftmax_rows(orx_ctx* ctx, const SampledSoftmaxArgs& a, bool query_grads) {
    {
        ProfScope ps(ctx, ORX_K_FUSED);
        ORX_LAUNCH(ctx, ss_gather_kernel, dim3((unsigned)((a.Bp + a.Sp + 3) / 4)), dim3(256), 0, a);
        ORX_HIP(hipGetLastError());
    }
    ProfScope ps(ctx, ORX_K_GEMM);
    return query_grads ? ss_rows<true>(ctx, a) : ss_rows<false>(ctx, a);
}

int orx_launch_sampledsoftmax_cols(orx_ctx* ctx, const SampledSoftmaxArgs& a) {
    if (a.S == 0) return ORX_OK;
    {
        ProfScope ps(ctx, ORX_K_GEMM);
        CHECK(ss_cols(ctx, a));
    }
    ProfScope ps(ctx, ORX_K_FUSED);
    ORX_LAUNCH(ctx, ss_finish_kernel, dim3((unsigned)(((int64_t)a.S * a.gs + 255) / 256)), dim3(256), 0, a);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}
