// Conjugate gradient for the ALS half-step of WRMF (orx_als_half_step_cg) and the objective the half-steps descend
// (orx_als_objective); api_csr.hip has the entry points, include/openrec_hip.h the contract, kernels_als.hip the notation.
//
// A row never forms A_r.  One product A v = b (G v) + reg v + sum_j (c_j - b) (f_j . v) f_j is
//   gram      G v from the full square of G (als_gram_kernel's tiles mirrored across the diagonal by als_cg_square_kernel), lane d
//             holding element d (and d + 64 when D > 64) and walking row d of G four columns per ds_read_b128 against a broadcast
//             read of v: one fmaf chain over k per element;
//   entries   the row's entries in chunks of CH = 32 (D <= 64) or 16 gathered rows of F in the wavefront's own LDS, at a pitch = 4
//             (mod 64) words.  dot phase: lane (j, h) sums section h of f_j . v, the 2 (4) sections are added by a fixed butterfly;
//             axpy phase: lane d adds (c_j - b) s_j f_j[d] entry by entry.  No reduction across lanes per entry, no float atomics.
// ONE WAVEFRONT PER ROW: the CG vectors x, r (fp64) and p (fp32) live in registers, the scalars rs, p . Ap, alpha, beta are fp64 and
// their D-length sums a fixed butterfly over the 64 lanes.  A workgroup of 16 (8) wavefronts shares G in LDS and walks rows with a
// grid stride.
//
// Code paths, by the row's length n and D alone (orx_als_cg_row_breaks):
//   n <= CH        the gathered entries stay in LDS across the cg_steps + 1 products;
//   n <= ALS_SEG   they are streamed again for every product;
//   n >  ALS_SEG   the row is cut into segments of ALS_SEG entries.  als_cg_plan_kernel gives it a state slot and one scratch slot per
//                  segment; per product als_cg_long_partial_kernel forms every segment's partial -- from zero, one wavefront each,
//                  over the whole device -- and als_cg_long_update_kernel adds them IN SEGMENT ORDER and takes the CG step.  A long
//                  row that got no slots (scratch budget) is walked by its own wavefront in als_cg_rows_kernel with the very
//                  statements of the partial kernel, segment by segment: the same bits.
// Every shared statement is an explicit fma / fmaf or a lone product, so no two kernels contract it differently.
//
// The objective: both grams by als_gram_kernel (slab partials, added here in fp64 in slab order), the observed cells by one
// wavefront per OBJ_EPW consecutive entries of the CSR (the dot product summed in fp64 by the butterfly), one workgroup adds
// everything in fp64 in a fixed order.
#include "orx_als.h"

constexpr int OBJ_EPW = 256;       // entries per wavefront of the objective's pass
constexpr int OBJ_B = 8;           // of them in flight
constexpr int OBJ_THREADS = 1024;

template <int NE>
struct CgGeom {
    static constexpr int Dp = 64 * NE;
    static constexpr int CH = 32 / NE;                 // entries per chunk
    static constexpr int LPE = 64 / CH;                // lanes per entry in the dot phase
    static constexpr int DSEC = Dp / LPE;              // elements of a dot section
    static constexpr int PITCH = Dp + 4;               // = 4 (mod 64) words: the 16 lanes of a ds_read_b128 group fall into 64 banks
    static constexpr int GB = 16 / NE;                 // gathered rows in flight per wavefront (CH is a multiple)
    static constexpr int WAVES = NE == 1 ? 16 : 8;     // G (16 / 64 KiB) + WAVES chunks: 150 / 133 KiB, one workgroup per CU
    static constexpr int THREADS = 64 * WAVES;
    static constexpr int WLDS = CH * PITCH + Dp;       // floats of a wavefront's chunk and its copy of v
};

int orx_als_cg_breaks(int D, int32_t* out, int cap) {
    if (D < 1 || D > 128) return 0;
    const int32_t b[2] = {D <= 64 ? CgGeom<1>::CH : CgGeom<2>::CH, ALS_SEG};
    for (int i = 0; i < 2 && i < cap; ++i) out[i] = b[i];
    return 2;
}
int64_t orx_als_cg_slot_floats(int D) { return 2 * (D <= 64 ? 64 : 128); }
int64_t orx_als_cg_square_floats(int D) { const int Dp = D <= 64 ? 64 : 128; return (int64_t)Dp * (Dp + 4); }
int64_t orx_als_cg_state_bytes(int D) { return (int64_t)(D <= 64 ? 64 : 128) * 20; }      // x, r fp64 and p fp32 per element

__device__ __forceinline__ void cg_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ float cg_lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
// the sum of the 64 lanes' values, the same bits in every lane
__device__ __forceinline__ double cg_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// out += sum over the entries [e0, e1) of (c - b) (f . v) f, y += sum c f (WITH_Y); one wavefront, v in vs[Dp] (LDS), chunk in fs
template <int NE, bool WITH_Y>
__device__ __forceinline__ void cg_segment(float* fs, const float* vs, const CgArgs& p, int64_t e0, int64_t e1, bool gather,
                                           float (&out)[NE], float (&y)[NE]) {
    using G = CgGeom<NE>;
    const int lane = threadIdx.x & 63, j = lane & (G::CH - 1), h = lane / G::CH;
    for (int64_t c0 = e0; c0 < e1; c0 += G::CH) {
        const int cnt = (int)((e1 - c0) < G::CH ? (e1 - c0) : G::CH);
        int col = -1; float c = 0.f, w = 0.f;
        if (j < cnt) {
            col = p.cols[c0 + j];
            if ((uint32_t)col >= (uint64_t)p.M) { *p.err = 1; col = -1; }
            else { c = p.conf ? p.conf[c0 + j] : p.a; w = c - p.b; }
        }
        if (gather) {
            cg_wave_sync();                                // the previous chunk has been consumed
            // GB rows at a time, their loads ahead of their stores; rows cnt .. of the last batch are stored as zeros
            for (int k0 = 0; k0 < cnt; k0 += G::GB) {
                float f[G::GB][NE];
#pragma unroll
                for (int u = 0; u < G::GB; ++u) {
                    const int ck = __builtin_amdgcn_readlane(col, k0 + u);      // -1 from entry cnt on
#pragma unroll
                    for (int e = 0; e < NE; ++e) {
                        const int d = lane + 64 * e;
                        f[u][e] = ck >= 0 && d < p.D ? p.F[(size_t)ck * p.D + d] : 0.f;
                    }
                }
#pragma unroll
                for (int u = 0; u < G::GB; ++u)
#pragma unroll
                    for (int e = 0; e < NE; ++e) fs[(k0 + u) * G::PITCH + lane + 64 * e] = f[u][e];
            }
            cg_wave_sync();
        }
        // dot phase: lane (j, h) sums elements [h DSEC, (h + 1) DSEC) of f_j . v; columns D .. Dp - 1 are zeros on both sides
        float s = 0.f;
        const float4* fr = reinterpret_cast<const float4*>(fs + j * G::PITCH + h * G::DSEC);
        const float4* vr = reinterpret_cast<const float4*>(vs + h * G::DSEC);
#pragma unroll
        for (int i = 0; i < G::DSEC / 4; ++i) {
            const float4 f = fr[i], v = vr[i];
            s = fmaf(f.x, v.x, s); s = fmaf(f.y, v.y, s); s = fmaf(f.z, v.z, s); s = fmaf(f.w, v.w, s);
        }
#pragma unroll
        for (int m = G::CH; m < 64; m <<= 1) s += __shfl_xor(s, m);
        const float ws = w * s;
        // axpy phase: lane d, entry by entry
        for (int k = 0; k < cnt; ++k) {
            const float wk = cg_lane_f(ws, k);
            const float ck = WITH_Y ? cg_lane_f(c, k) : 0.f;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const float f = fs[k * G::PITCH + lane + 64 * e];
                out[e] = fmaf(wk, f, out[e]);
                if (WITH_Y) y[e] = fmaf(ck, f, y[e]);
            }
        }
    }
}

// gv = G v: Gsrc [Dp][PITCH] in LDS or in HBM (G is symmetric: lane d walks ITS row, four columns per load), v in vs[Dp]; element d is
// one fmaf chain over k ascending
template <int NE>
__device__ __forceinline__ void cg_gram(const float* Gsrc, const float* vs, int D, float (&gv)[NE]) {
    using G = CgGeom<NE>;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int e = 0; e < NE; ++e) gv[e] = 0.f;
    for (int k0 = 0; k0 < D; k0 += 4) {                    // columns D .. are zeros on both sides
        const float4 v = *reinterpret_cast<const float4*>(vs + k0);
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const float4 g = *reinterpret_cast<const float4*>(Gsrc + (size_t)(lane + 64 * e) * G::PITCH + k0);
            gv[e] = fmaf(g.x, v.x, gv[e]); gv[e] = fmaf(g.y, v.y, gv[e]); gv[e] = fmaf(g.z, v.z, gv[e]); gv[e] = fmaf(g.w, v.w, gv[e]);
        }
    }
}

template <int NE>
struct CgState { double x[NE], r[NE]; float p[NE]; double rs; };

template <int NE>
__device__ __forceinline__ double cg_dot(const double (&u)[NE], const double (&v)[NE]) {
    double t = u[0] * v[0];
#pragma unroll
    for (int e = 1; e < NE; ++e) t = fma(u[e], v[e], t);
    return cg_wave_sum(t);
}

// Av = b (G v) + reg v + tot
template <int NE>
__device__ __forceinline__ void cg_combine(const CgArgs& p, const float (&gv)[NE], const float (&v)[NE], const float (&tot)[NE], float (&Av)[NE]) {
#pragma unroll
    for (int e = 0; e < NE; ++e) Av[e] = fmaf(p.b, gv[e], fmaf(p.reg, v[e], tot[e]));
}

// x = the row's current value; r = y - A x; p = r; rs = r . r
template <int NE>
__device__ __forceinline__ void cg_init(CgState<NE>& st, const float (&x)[NE], const float (&y)[NE], const float (&Ax)[NE]) {
#pragma unroll
    for (int e = 0; e < NE; ++e) { st.x[e] = (double)x[e]; st.r[e] = (double)y[e] - (double)Ax[e]; st.p[e] = (float)st.r[e]; }
    st.rs = cg_dot<NE>(st.r, st.r);
}

// one CG step with Ap = A p.  rs <= 1e-20 freezes the row by a select (NaN compares false and flows through)
template <int NE>
__device__ __forceinline__ void cg_step(CgState<NE>& st, const float (&Ap)[NE]) {
    double pd[NE], apd[NE], xn[NE], rn[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) { pd[e] = (double)st.p[e]; apd[e] = (double)Ap[e]; }
    const bool done = st.rs <= 1e-20;
    const double alpha = st.rs / cg_dot<NE>(pd, apd);
#pragma unroll
    for (int e = 0; e < NE; ++e) { xn[e] = fma(alpha, pd[e], st.x[e]); rn[e] = fma(-alpha, apd[e], st.r[e]); }
    const double rsn = cg_dot<NE>(rn, rn);
    const double beta = rsn / st.rs;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const float pn = (float)fma(beta, pd[e], rn[e]);
        st.x[e] = done ? st.x[e] : xn[e]; st.r[e] = done ? st.r[e] : rn[e]; st.p[e] = done ? st.p[e] : pn;
    }
    st.rs = done ? st.rs : rsn;
}

// v goes to the wavefront's LDS copy (the dot phase reads it by section)
template <int NE>
__device__ __forceinline__ void cg_publish(float* vs, const float (&v)[NE]) {
    const int lane = threadIdx.x & 63;
    cg_wave_sync();
#pragma unroll
    for (int e = 0; e < NE; ++e) vs[lane + 64 * e] = v[e];
    cg_wave_sync();
}

// the whole solve of one row by one wavefront
template <int NE>
__device__ __forceinline__ void cg_row(const CgArgs& p, const float* Gsrc, float* fs, float* vs, int64_t row) {
    using G = CgGeom<NE>;
    const int lane = threadIdx.x & 63, D = p.D;
    const int64_t r0 = p.rp[row], r1 = p.rp[row + 1];
    float* xrow = p.X + (size_t)row * D;
    if (r1 <= r0) {                                        // no observation: the system's solution is zero
#pragma unroll
        for (int e = 0; e < NE; ++e) if (lane + 64 * e < D) xrow[lane + 64 * e] = 0.f;
        return;
    }
    const int64_t n = r1 - r0, nseg = (n + ALS_SEG - 1) / ALS_SEG;
    const bool resident = n <= G::CH;
    float x0[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) x0[e] = lane + 64 * e < D ? xrow[lane + 64 * e] : 0.f;
    CgState<NE> st;
    for (int it = 0; it <= p.cg_steps; ++it) {
        float v[NE], tot[NE], ytot[NE], gv[NE], Av[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) { v[e] = it == 0 ? x0[e] : st.p[e]; tot[e] = 0.f; ytot[e] = 0.f; }
        cg_publish<NE>(vs, v);
        for (int64_t sg = 0; sg < nseg; ++sg) {            // segment order, each partial from zero
            const int64_t e0 = r0 + sg * ALS_SEG, e1 = e0 + ALS_SEG < r1 ? e0 + ALS_SEG : r1;
            float part[NE], yp[NE];
#pragma unroll
            for (int e = 0; e < NE; ++e) { part[e] = 0.f; yp[e] = 0.f; }
            if (it == 0) cg_segment<NE, true>(fs, vs, p, e0, e1, true, part, yp);
            else cg_segment<NE, false>(fs, vs, p, e0, e1, !resident, part, yp);
#pragma unroll
            for (int e = 0; e < NE; ++e) { tot[e] += part[e]; ytot[e] += yp[e]; }
        }
        cg_gram<NE>(Gsrc, vs, D, gv);
        cg_combine<NE>(p, gv, v, tot, Av);
        if (it == 0) cg_init<NE>(st, x0, ytot, Av);
        else cg_step<NE>(st, Av);
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) if (lane + 64 * e < D) xrow[lane + 64 * e] = (float)st.x[e];
}

// Gq[d][k] = G(d, k) for d, k < D, zero elsewhere in [Dp][pitch], from the tiles on and below the diagonal of Gm [Dp16][Dp16]
__global__ __launch_bounds__(256) void als_cg_square_kernel(const float* __restrict__ Gm, int D, int Dp16, int Dp, int pitch, float* __restrict__ Gq) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Dp * pitch) return;
    const int d = e / pitch, k = e % pitch;
    float v = 0.f;
    if (d < D && k < D) v = (d >> 4) >= (k >> 4) ? Gm[d * Dp16 + k] : Gm[k * Dp16 + d];
    Gq[e] = v;
}

template <int NE>
__global__ __launch_bounds__(CgGeom<NE>::THREADS) void als_cg_rows_kernel(CgArgs p) {
    using G = CgGeom<NE>;
    extern __shared__ __attribute__((aligned(16))) float cg_lds[];
    float* Gs = cg_lds;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* fs = cg_lds + G::Dp * G::PITCH + wave * G::WLDS;
    float* vs = fs + G::CH * G::PITCH;
    for (int idx = threadIdx.x; idx < G::Dp * G::PITCH; idx += G::THREADS) Gs[idx] = p.Gq[idx];
    __syncthreads();
    for (int64_t row = (int64_t)blockIdx.x * G::WAVES + wave; row < p.nrows; row += (int64_t)gridDim.x * G::WAVES) {
        if (p.long_idx && p.long_idx[row] >= 0) continue;  // the long-row kernels solve it
        cg_row<NE>(p, Gs, fs, vs, row);
    }
}

// ------------------------------------------------------------------------------------- long rows ---
// One thread per row of the call: a row of more than ALS_SEG entries takes one state slot and nseg consecutive scratch slots (integer
// counters: the slot NUMBERS depend on the launch, what is written into a slot does not); a row that does not fit gets none.
__global__ __launch_bounds__(256) void als_cg_plan_kernel(const int64_t* __restrict__ rp, int64_t nrows, int cap_rows, int cap_slots,
                                                          unsigned long long* __restrict__ counter, int* __restrict__ long_idx,
                                                          int2* __restrict__ rowlist, int2* __restrict__ list) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrows) return;
    const int64_t n = rp[i + 1] - rp[i];
    int idx = -1;
    if (n > ALS_SEG) {
        const int64_t nseg64 = (n + ALS_SEG - 1) / ALS_SEG;
        if (nseg64 <= cap_slots) {
            const unsigned long long nseg = (unsigned long long)nseg64;
            const unsigned long long got = atomicAdd(counter, (1ull << 32) | nseg);      // 32 bits of slots: never carries into the rows
            const unsigned long long ri = got >> 32, base = got & 0xffffffffull;
            if (ri < (unsigned long long)cap_rows && base + nseg <= (unsigned long long)cap_slots) {
                idx = (int)ri;
                rowlist[ri] = make_int2((int)i, (int)base);
                for (int sg = 0; sg < (int)nseg; ++sg) list[base + sg] = make_int2(idx, sg);
            } else {
                if (ri < (unsigned long long)cap_rows) rowlist[ri] = make_int2(-1, -1);
                for (unsigned long long sg = base; sg < base + nseg && sg < (unsigned long long)cap_slots; ++sg) list[sg] = make_int2(-1, -1);
            }
        }
    }
    long_idx[i] = idx;
}

// product `it` of the long rows, one wavefront per segment: v = the row's current value (it == 0) or its p
template <int NE>
__global__ __launch_bounds__(CgGeom<NE>::THREADS) void als_cg_long_partial_kernel(CgArgs p, int it) {
    using G = CgGeom<NE>;
    extern __shared__ __attribute__((aligned(16))) float cg_lds[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    float* fs = cg_lds + wave * G::WLDS;
    float* vs = fs + G::CH * G::PITCH;
    const unsigned long long used = *p.counter & 0xffffffffull;
    const int count = used < (unsigned long long)p.cap_slots ? (int)used : p.cap_slots;
    const int slot = blockIdx.x * G::WAVES + wave;
    if (slot >= count) return;
    const int2 w = p.list[slot];
    if (w.x < 0) return;
    const int64_t row = p.rowlist[w.x].x;
    const int64_t r0 = p.rp[row], r1 = p.rp[row + 1];
    const int64_t e0 = r0 + (int64_t)w.y * ALS_SEG, e1 = e0 + ALS_SEG < r1 ? e0 + ALS_SEG : r1;
    float v[NE], part[NE], yp[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int d = lane + 64 * e;
        v[e] = it == 0 ? (d < p.D ? p.X[(size_t)row * p.D + d] : 0.f) : p.sp[(size_t)w.x * G::Dp + d];
        part[e] = 0.f; yp[e] = 0.f;
    }
    cg_publish<NE>(vs, v);
    if (it == 0) cg_segment<NE, true>(fs, vs, p, e0, e1, true, part, yp);
    else cg_segment<NE, false>(fs, vs, p, e0, e1, true, part, yp);
    float* out = p.slots + (size_t)slot * 2 * G::Dp;
#pragma unroll
    for (int e = 0; e < NE; ++e) { out[lane + 64 * e] = part[e]; out[G::Dp + lane + 64 * e] = yp[e]; }
}

// the CG statement that follows product `it`, one wavefront per long row; after the last one x is stored
template <int NE>
__global__ __launch_bounds__(256) void als_cg_long_update_kernel(CgArgs p, int it) {
    using G = CgGeom<NE>;
    __shared__ __attribute__((aligned(16))) float vsh[4][G::Dp];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const unsigned long long used = *p.counter >> 32;
    const int count = used < (unsigned long long)p.cap_rows ? (int)used : p.cap_rows;
    const int ri = blockIdx.x * 4 + wave;
    if (ri >= count) return;
    const int2 w = p.rowlist[ri];
    if (w.x < 0) return;
    const int64_t row = w.x;
    const int64_t n = p.rp[row + 1] - p.rp[row], nseg = (n + ALS_SEG - 1) / ALS_SEG;
    float* xrow = p.X + (size_t)row * p.D;
    const size_t so = (size_t)ri * G::Dp;
    CgState<NE> st;
    float v[NE], tot[NE], ytot[NE], gv[NE], Av[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int d = lane + 64 * e;
        if (it == 0) v[e] = d < p.D ? xrow[d] : 0.f;
        else { st.x[e] = p.sx[so + d]; st.r[e] = p.sr[so + d]; st.p[e] = p.sp[so + d]; v[e] = st.p[e]; }
        tot[e] = 0.f; ytot[e] = 0.f;
    }
    if (it != 0) st.rs = p.srs[ri];
    for (int64_t sg = 0; sg < nseg; ++sg) {                // segment order
        const float* in = p.slots + (size_t)(w.y + sg) * 2 * G::Dp;
#pragma unroll
        for (int e = 0; e < NE; ++e) { tot[e] += in[lane + 64 * e]; ytot[e] += in[G::Dp + lane + 64 * e]; }
    }
    cg_publish<NE>(vsh[wave], v);
    cg_gram<NE>(p.Gq, vsh[wave], p.D, gv);
    cg_combine<NE>(p, gv, v, tot, Av);
    if (it == 0) cg_init<NE>(st, v, ytot, Av);
    else cg_step<NE>(st, Av);
    if (it == p.cg_steps) {
#pragma unroll
        for (int e = 0; e < NE; ++e) if (lane + 64 * e < p.D) xrow[lane + 64 * e] = (float)st.x[e];
        return;
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) { const int d = lane + 64 * e; p.sx[so + d] = st.x[e]; p.sr[so + d] = st.r[e]; p.sp[so + d] = st.p[e]; }
    if (lane == 0) p.srs[ri] = st.rs;
}

template <int NE>
static int als_cg_launch_NE(orx_ctx* ctx, const CgArgs& p, bool plan) {
    using G = CgGeom<NE>;
    const size_t lds_rows = (size_t)(G::Dp * G::PITCH + G::WAVES * G::WLDS) * sizeof(float), lds_long = (size_t)G::WAVES * G::WLDS * sizeof(float);
    ORX_ONCE_PER_DEVICE(ctx, ORX_HIP(hipFuncSetAttribute((const void*)als_cg_rows_kernel<NE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_rows)));
    ORX_ONCE_PER_DEVICE(ctx, ORX_HIP(hipFuncSetAttribute((const void*)als_cg_long_partial_kernel<NE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_long)));
    const int64_t need = (p.nrows + G::WAVES - 1) / G::WAVES, most = (int64_t)ctx->num_cu * 4;
    ORX_LAUNCH(ctx, als_cg_rows_kernel<NE>, dim3((unsigned)(need < most ? need : most)), dim3(G::THREADS), lds_rows, p);
    if (plan) {
        for (int it = 0; it <= p.cg_steps; ++it) {
            ORX_LAUNCH(ctx, als_cg_long_partial_kernel<NE>, dim3((unsigned)((p.cap_slots + G::WAVES - 1) / G::WAVES)), dim3(G::THREADS), lds_long, p, it);
            ORX_LAUNCH(ctx, als_cg_long_update_kernel<NE>, dim3((unsigned)((p.cap_rows + 3) / 4)), dim3(256), 0, p, it);
        }
    }
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

// the CG half-step on the context's stream, Gm (als_gram_kernel + als_gram_reduce_kernel) already enqueued
int orx_launch_als_cg(orx_ctx* ctx, CgArgs p, const float* Gm, float* Gq, unsigned long long* counter, int* long_idx, int2* rowlist, int2* list) {
    const int D = p.D, Dp = D <= 64 ? 64 : 128, Dp16 = (D + 15) / 16 * 16;
    ORX_LAUNCH(ctx, als_cg_square_kernel, dim3((Dp * (Dp + 4) + 255) / 256), dim3(256), 0, Gm, D, Dp16, Dp, Dp + 4, Gq);
    p.Gq = Gq; p.err = ctx->d_err;
    const bool plan = p.cap_slots > 0 && p.cap_rows > 0;
    p.long_idx = plan ? long_idx : nullptr; p.rowlist = rowlist; p.list = list; p.counter = counter;
    if (plan) {
        ORX_HIP(hipMemsetAsync(counter, 0, sizeof(unsigned long long), ctx->stream));
        ORX_LAUNCH(ctx, als_cg_plan_kernel, dim3((unsigned)((p.nrows + 255) / 256)), dim3(256), 0, p.rp, p.nrows, p.cap_rows, p.cap_slots, counter,
                   long_idx, rowlist, list);
    }
    return D <= 64 ? als_cg_launch_NE<1>(ctx, p, plan) : als_cg_launch_NE<2>(ctx, p, plan);
}

// --------------------------------------------------------------------------------------- objective ---
// sum over the entries [w OBJ_EPW, (w + 1) OBJ_EPW) of c (1 - s)^2 - b s^2, s = u . v summed in fp64, in entry order; OBJ_B entries at a
// time, their loads ahead of their sums
__global__ __launch_bounds__(256) void als_obj_entries_kernel(ObjArgs p) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + wave;
    if (w >= p.nw) return;
    const int64_t e0 = w * OBJ_EPW, e1 = e0 + OBJ_EPW < p.nnz ? e0 + OBJ_EPW : p.nnz;
    int64_t lo = 0, hi = p.NU;                             // the row of entry e0: the last one with rp[row] <= e0
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (p.rp[mid] <= e0) lo = mid; else hi = mid;
    }
    int64_t row = lo, next = p.rp[row + 1];
    double acc = 0.0;
    for (int64_t eb = e0; eb < e1; eb += OBJ_B) {
        double t[OBJ_B]; float c[OBJ_B]; bool ok[OBJ_B];
#pragma unroll
        for (int k = 0; k < OBJ_B; ++k) {
            const int64_t e = eb + k;
            ok[k] = e < e1;
            t[k] = 0.0; c[k] = 0.f;
            if (ok[k]) {
                while (row + 1 < p.NU && e >= next) { ++row; next = p.rp[row + 1]; }
                const int col = p.cols[e];
                if ((uint32_t)col >= (uint64_t)p.NI) { *p.err = 1; ok[k] = false; }
                else {
                    c[k] = p.conf ? p.conf[e] : p.a;
#pragma unroll
                    for (int q = 0; q < 2; ++q)
                        if (lane + 64 * q < p.D)
                            t[k] = fma((double)p.U[(size_t)row * p.D + lane + 64 * q], (double)p.V[(size_t)col * p.D + lane + 64 * q], t[k]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < OBJ_B; ++k) {
            const double s = cg_wave_sum(t[k]);
            if (ok[k]) acc += (double)c[k] * (1.0 - s) * (1.0 - s) - (double)p.b * s * s;
        }
    }
    if (lane == 0) p.part[w] = acc;
}

// 256 elements of the Dp16 x Dp16 square per workgroup, the slabs of both grams added in fp64 in slab order:
// gpart[2 g] = sum of G_U(i, j) G_V(i, j) (twice below the diagonal tiles: the tiles above them were not formed), gpart[2 g + 1] =
// sum over the diagonal of G_U + G_V
__global__ __launch_bounds__(256) void als_obj_gram_kernel(ObjArgs p) {
    __shared__ double red[2][256];
    const int tid = threadIdx.x, n = p.Dp16 * p.Dp16, e = blockIdx.x * 256 + tid;
    double g = 0.0, t = 0.0;
    if (e < n) {
        const int i = e / p.Dp16, j = e % p.Dp16;
        if ((i >> 4) >= (j >> 4)) {
            double gu = 0.0, gv = 0.0;
            for (int s = 0; s < p.nbU; ++s) gu += (double)p.gramU[(size_t)s * n + e];
            for (int s = 0; s < p.nbV; ++s) gv += (double)p.gramV[(size_t)s * n + e];
            g = ((i >> 4) > (j >> 4) ? 2.0 : 1.0) * gu * gv;
            if (i == j) t = gu + gv;
        }
    }
    red[0][tid] = g; red[1][tid] = t;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if (tid < m) { red[0][tid] += red[0][tid + m]; red[1][tid] += red[1][tid + m]; }
        __syncthreads();
    }
    if (tid == 0) { p.gpart[2 * blockIdx.x] = red[0][0]; p.gpart[2 * blockIdx.x + 1] = red[1][0]; }
}

// one workgroup: b <G_U, G_V>_F + the entries' partials + reg (tr G_U + tr G_V), every sum in fp64 in a fixed order
__global__ __launch_bounds__(OBJ_THREADS) void als_obj_final_kernel(ObjArgs p) {
    __shared__ double red[OBJ_THREADS];
    const int tid = threadIdx.x;
    double v = 0.0;
    for (int64_t w = tid; w < p.nw; w += OBJ_THREADS) v += p.part[w];
    if (tid < p.ngw) v += (double)p.b * p.gpart[2 * tid] + (double)p.reg * p.gpart[2 * tid + 1];
    red[tid] = v;
    __syncthreads();
    for (int m = OBJ_THREADS / 2; m >= 1; m >>= 1) {
        if (tid < m) red[tid] += red[tid + m];
        __syncthreads();
    }
    if (tid == 0) *p.out = red[0];
}

int orx_als_obj_gram_groups(int D) { const int Dp16 = (D + 15) / 16 * 16; return (Dp16 * Dp16 + 255) / 256; }      // <= 64
int64_t orx_als_obj_waves(int64_t nnz) { return (nnz + OBJ_EPW - 1) / OBJ_EPW; }

int orx_launch_als_objective(orx_ctx* ctx, ObjArgs p) {
    p.err = ctx->d_err;
    if (p.nw > 0) ORX_LAUNCH(ctx, als_obj_entries_kernel, dim3((unsigned)((p.nw + 3) / 4)), dim3(256), 0, p);
    ORX_LAUNCH(ctx, als_obj_gram_kernel, dim3(p.ngw), dim3(256), 0, p);
    ORX_LAUNCH(ctx, als_obj_final_kernel, dim3(1), dim3(OBJ_THREADS), 0, p);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}
