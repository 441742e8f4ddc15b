// Alternating least squares for WRMF (orx_als_half_step, api_csr.hip): with one table F [M, D] held fixed, every row x_r of the
// other table solves
//     A_r x_r = y_r,   A_r = b G + sum_{j in O_r} (c_rj - b) f_j f_j^T + reg I,   y_r = sum_{j in O_r} c_rj f_j,   G = F^T F
// in closed form (Hu / Koren / Volinsky 2008).  Three kernels, fp32 throughout, no float atomics anywhere:
//
//   gram      als_gram_kernel<T>: G = F^T F.  The rows of F are cut into als_gram_blocks(M) equal slabs (a function of M alone), one
//             workgroup per slab; a slab's partial G stays in MFMA accumulators and goes to scratch, als_gram_reduce_kernel adds the
//             partials in slab order.
//   segments  seg_plan_kernel<ALS_SEG> (orx_seg_plan.h) + als_segment_kernel<T>: a row of more than ALS_SEG entries is cut into
//             segments of ALS_SEG entries (the last one shorter); one workgroup per segment writes its partial (A, y) -- started
//             from zero -- to a scratch slot.
//   solve     als_solve_kernel<T>: one workgroup per row.  total = sum over the row's segments IN SEGMENT ORDER of the segment's
//             partial, read from its slot or, where the row got no slots (scratch budget) or has one segment only, formed from zero by
//             the workgroup itself with the very statements of the segment kernel: the bits of x_r are a function of the row alone,
//             never of the launch, the budget or the other rows of the call.  Then A = total + b G + reg I goes to LDS in fp64 as a
//             PACKED lower triangle, is factorised (Cholesky, right-looking, one barrier per column, the forward substitution riding
//             along), back-substituted, and x_r is rounded to fp32 once and stored.
//
// Precision.  The sums (G, the rank updates, y) are fp32 on the matrix cores; the factorisation and the substitutions are fp64.  With
// them in fp32 the solve alone put up to 1e-6 of error on well-conditioned rows (reg = 10, D = 128) where forming A and y in fp32
// costs 2e-7: nine times NumPy's float32 solve on the worst test case.  In fp64 the solve adds nothing visible.
//
// Tiles.  Dp = 16 T is D rounded up to the 16 x 16 x 4 fp32 MFMA tile (T = 1 .. 8).  Only the T (T + 1) / 2 tiles on and below the
// diagonal are formed, dealt round-robin to the workgroup's four wavefronts (at most 9 tiles = 36 accumulator registers each).  A
// chunk of ALS_CH gathered rows of F sits in LDS at a pitch = 16 (mod 64) words, so the 4 x 16 words a wavefront reads for one
// operand fall into 64 distinct banks; columns D .. Dp - 1 and entries past the chunk's end are zeros with weight zero.  The
// padded rows and columns never reach the factorisation: it runs over the D x D corner only.
//
// LDS.  The chunk (ALS_CH x pitch words) and the packed fp64 triangle (Dp (Dp + 1) / 2 doubles) are never live together and share
// one region: 64.5 KiB at D = 128 -- the full fp64 square would be 128 KiB --, 16.3 KiB at D = 64; with the vectors 69.5 KiB / 18.8
// KiB per workgroup: 2 workgroups (8 wavefronts) per CU at D = 128; at D <= 64 registers, not LDS, set the limit (5 workgroups).
//
// Non-finite inputs give non-finite x_r: every loop's trip count is an integer function of D and the row's length.
#include "orx_als.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int ALS_CH = 32;         // gathered rows of F per LDS chunk
constexpr int ALS_WAVES = 4;
constexpr int ALS_THREADS = 64 * ALS_WAVES;

template <int T>
struct AlsGeom {
    static constexpr int Dp = 16 * T;
    static constexpr int PITCH = ((Dp + 47) / 64) * 64 + 16;      // >= Dp, = 16 (mod 64)
    static constexpr int NT = T * (T + 1) / 2;                    // tiles on and below the diagonal
    static constexpr int MAXT = (NT + ALS_WAVES - 1) / ALS_WAVES; // tiles per wavefront
    static constexpr int TRI = Dp * (Dp + 1) / 2;
    static constexpr int SLOT = Dp * Dp + Dp;                     // floats of a partial (A as a Dp x Dp square, then y)
};

int64_t orx_als_slot_floats(int D) { const int Dp = (D + 15) / 16 * 16; return (int64_t)Dp * Dp + Dp; }

// what the accumulation of a run of entries needs in LDS
template <int T>
struct AlsLds {
    float region[ALS_CH * AlsGeom<T>::PITCH];      // the chunk [ALS_CH][PITCH]
    int col[ALS_CH];
    float wsub[ALS_CH];                    // c - b (0 for an absent entry)
    float wc[ALS_CH];                      // c
};

__device__ __forceinline__ void als_tile_of(int q, int& ti, int& tj) {
    ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= q) ++ti;
    tj = q - ti * (ti + 1) / 2;
}

// acc[t] += sum_k w_k f_k f_k^T over the tiles of this wavefront, yv += sum_k c_k f_k[tid] (threads tid < Dp), for the entries
// [e0, e1) of one row.  GATHER: entry e is row cols[e] of F with confidence conf[e] (NULL: a); else entry e is row e of F, weight 1
// (the gram).  Chunks of ALS_CH entries in ascending order; inside a chunk the MFMA k order, then y in entry order.
template <int T, bool GATHER>
__device__ __forceinline__ void als_accumulate(AlsLds<T>& s, const float* __restrict__ F, int64_t M, int D,
                                               const int32_t* __restrict__ cols, const float* __restrict__ conf, float a, float b,
                                               int64_t e0, int64_t e1, f32x4 (&acc)[AlsGeom<T>::MAXT], float& yv, int* err) {
    using G = AlsGeom<T>;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool vec = (D & 3) == 0;
    int oa[G::MAXT], ob[G::MAXT];                          // column offsets of this wavefront's tiles
#pragma unroll
    for (int t = 0; t < G::MAXT; ++t) {
        int ti, tj;
        als_tile_of(wave + ALS_WAVES * t < G::NT ? wave + ALS_WAVES * t : 0, ti, tj);
        oa[t] = 16 * ti; ob[t] = 16 * tj;
    }
    for (int64_t c0 = e0; c0 < e1; c0 += ALS_CH) {
        const int cnt = (int)((e1 - c0) < ALS_CH ? (e1 - c0) : ALS_CH);
        __syncthreads();                                   // the previous chunk has been consumed
        if (tid < ALS_CH) {
            int col = -1; float c = 0.f, w = 0.f;
            if (tid < cnt) {
                if (GATHER) {
                    col = cols[c0 + tid];
                    if ((uint32_t)col >= (uint64_t)M) { *err = 1; col = -1; }
                    else { c = conf ? conf[c0 + tid] : a; w = c - b; }
                } else {
                    col = 0; c = 1.f; w = 1.f;
                }
            }
            s.col[tid] = col; s.wsub[tid] = w; s.wc[tid] = c;
        }
        __syncthreads();
        if (vec) {
            for (int idx = tid; idx < ALS_CH * (G::Dp / 4); idx += ALS_THREADS) {
                const int k = idx / (G::Dp / 4), c4 = (idx % (G::Dp / 4)) * 4;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                const int col = s.col[k];
                if (col >= 0 && c4 < D) {
                    const int64_t row = GATHER ? (int64_t)col : c0 + k;
                    v = *reinterpret_cast<const f32x4*>(F + (size_t)row * D + c4);
                }
                *reinterpret_cast<f32x4*>(&s.region[k * G::PITCH + c4]) = v;
            }
        } else {
            for (int idx = tid; idx < ALS_CH * G::Dp; idx += ALS_THREADS) {
                const int k = idx / G::Dp, c = idx % G::Dp;
                float v = 0.f;
                const int col = s.col[k];
                if (col >= 0 && c < D) {
                    const int64_t row = GATHER ? (int64_t)col : c0 + k;
                    v = F[(size_t)row * D + c];
                }
                s.region[k * G::PITCH + c] = v;
            }
        }
        __syncthreads();
#pragma unroll 2
        for (int k0 = 0; k0 < ALS_CH; k0 += 4) {
            const int k = k0 + (lane >> 4);
            const float w = s.wsub[k];
            const float* frow = &s.region[k * G::PITCH + (lane & 15)];
#pragma unroll
            for (int t = 0; t < G::MAXT; ++t) {
                if (wave + ALS_WAVES * t < G::NT)
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(frow[oa[t]] * w, frow[ob[t]], acc[t], 0, 0, 0);
            }
        }
        if (GATHER && tid < G::Dp) {
            for (int k = 0; k < cnt; ++k) yv = fmaf(s.wc[k], s.region[k * G::PITCH + tid], yv);
        }
    }
}

// acc[t][r] is element (16 ti + 4 (lane / 16) + r, 16 tj + lane % 16) of the Dp x Dp square
template <int T, class Fn>
__device__ __forceinline__ void als_for_each(Fn fn) {
    using G = AlsGeom<T>;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < G::MAXT; ++t) {
        const int q = wave + ALS_WAVES * t;
        if (q < G::NT) {
            int ti, tj;
            als_tile_of(q, ti, tj);
#pragma unroll
            for (int r = 0; r < 4; ++r) fn(t, r, 16 * ti + 4 * (lane >> 4) + r, 16 * tj + (lane & 15));
        }
    }
}

// ------------------------------------------------------------------------------------------- gram ---
int orx_als_gram_blocks(int64_t M) {
    const int64_t nb = (M + 4 * ALS_CH - 1) / (4 * ALS_CH);      // at least 128 rows per slab
    return (int)(nb < 1 ? 1 : nb > 512 ? 512 : nb);
}

template <int T>
__global__ __launch_bounds__(ALS_THREADS) void als_gram_kernel(const float* __restrict__ F, int64_t M, int D, float* __restrict__ part) {
    using G = AlsGeom<T>;
    __shared__ __attribute__((aligned(16))) AlsLds<T> s;
    const int64_t per = ((M + gridDim.x - 1) / gridDim.x + ALS_CH - 1) / ALS_CH * ALS_CH;
    int64_t e0 = (int64_t)blockIdx.x * per, e1 = e0 + per;
    if (e0 > M) e0 = M;
    if (e1 > M) e1 = M;
    f32x4 acc[G::MAXT];
#pragma unroll
    for (int t = 0; t < G::MAXT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float yv = 0.f;
    als_accumulate<T, false>(s, F, M, D, nullptr, nullptr, 1.f, 0.f, e0, e1, acc, yv, nullptr);
    float* out = part + (size_t)blockIdx.x * G::Dp * G::Dp;
    als_for_each<T>([&](int t, int r, int i, int j) { out[i * G::Dp + j] = acc[t][r]; });
}

// G[i][j] = the slabs' partials added in slab order, for the tiles on and below the diagonal; the other tiles are zero
__global__ __launch_bounds__(256) void als_gram_reduce_kernel(const float* __restrict__ part, int nb, int Dp, float* __restrict__ Gm) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Dp * Dp) return;
    const int i = e / Dp, j = e % Dp;
    float v = 0.f;
    if ((i >> 4) >= (j >> 4))
        for (int p = 0; p < nb; ++p) v += part[(size_t)p * Dp * Dp + e];
    Gm[e] = v;
}

// --------------------------------------------------------------------------------------- segments ---
struct AlsArgs {
    const float* F; int64_t M; int D;              // the fixed table
    const float* Gm;                               // [Dp][Dp] gram, tiles on and below the diagonal
    float* X;                                      // the solved table's row row0 (rows of D floats)
    const int64_t* rp;                             // [nrows + 1] offsets of the call's rows
    const int32_t* cols; const float* conf;        // entry e of the CSR is cols[e - ebase]: both pointers are already shifted by -ebase
    int64_t nrows;
    float a, b, reg;
    SegPlan plan;                                  // slots: [cap][SLOT]
    int* err;
};

template <int T>
__global__ __launch_bounds__(ALS_THREADS) void als_segment_kernel(AlsArgs p) {
    using G = AlsGeom<T>;
    __shared__ __attribute__((aligned(16))) AlsLds<T> s;
    const int count = seg_plan_count(p.plan);
    for (int it = blockIdx.x; it < count; it += gridDim.x) {
        const int2 w = p.plan.list[it];
        if (w.x < 0) continue;
        const int64_t r0 = p.rp[w.x], r1 = p.rp[w.x + 1];
        const int64_t e0 = r0 + (int64_t)w.y * ALS_SEG;
        const int64_t e1 = e0 + ALS_SEG < r1 ? e0 + ALS_SEG : r1;
        f32x4 acc[G::MAXT];
#pragma unroll
        for (int t = 0; t < G::MAXT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        float yv = 0.f;
        als_accumulate<T, true>(s, p.F, p.M, p.D, p.cols, p.conf, p.a, p.b, e0, e1, acc, yv, p.err);
        float* out = p.plan.slots + (size_t)it * G::SLOT;
        als_for_each<T>([&](int t, int r, int i, int j) { out[i * G::Dp + j] = acc[t][r]; });
        if (threadIdx.x < G::Dp) out[G::Dp * G::Dp + threadIdx.x] = yv;
    }
}

// ------------------------------------------------------------------------------------------ solve ---
template <int T>
__global__ __launch_bounds__(ALS_THREADS) void als_solve_kernel(AlsArgs p) {
    using G = AlsGeom<T>;
    // the chunk of the accumulation, later the packed triangle in fp64: never live together
    constexpr size_t RAW = sizeof(AlsLds<T>) > G::TRI * sizeof(double) ? sizeof(AlsLds<T>) : G::TRI * sizeof(double);
    __shared__ __attribute__((aligned(16))) unsigned char raw[RAW];
    __shared__ double ys[G::Dp], zs[G::Dp], dinv[G::Dp], lcol[2][G::Dp];
    AlsLds<T>& s = *reinterpret_cast<AlsLds<T>*>(raw);
    const int tid = threadIdx.x, ti = tid >> 4, tk = tid & 15;
    const int D = p.D;
    const int64_t row = blockIdx.x;
    const int64_t r0 = p.rp[row], r1 = p.rp[row + 1];
    float* x = p.X + (size_t)row * D;
    if (r1 <= r0) {                                        // no observation: the system's solution is zero
        if (tid < D) x[tid] = 0.f;
        return;
    }
    const int64_t n = r1 - r0;
    const int64_t nseg = (n + ALS_SEG - 1) / ALS_SEG;
    const int base = p.plan.seg_base ? p.plan.seg_base[row] : -1;
    f32x4 tot[G::MAXT];
#pragma unroll
    for (int t = 0; t < G::MAXT; ++t) tot[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float ytot = 0.f;
    for (int64_t sg = 0; sg < nseg; ++sg) {                // segment order, whoever formed the partial
        f32x4 acc[G::MAXT];
#pragma unroll
        for (int t = 0; t < G::MAXT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        float yv = 0.f;
        if (base >= 0) {
            const float* in = p.plan.slots + (size_t)(base + sg) * G::SLOT;
            als_for_each<T>([&](int t, int r, int i, int j) { acc[t][r] = in[i * G::Dp + j]; });
            if (tid < G::Dp) yv = in[G::Dp * G::Dp + tid];
        } else {
            const int64_t e0 = r0 + sg * ALS_SEG;
            const int64_t e1 = e0 + ALS_SEG < r1 ? e0 + ALS_SEG : r1;
            als_accumulate<T, true>(s, p.F, p.M, D, p.cols, p.conf, p.a, p.b, e0, e1, acc, yv, p.err);
        }
#pragma unroll
        for (int t = 0; t < G::MAXT; ++t) tot[t] += acc[t];
        ytot += yv;
    }
    __syncthreads();                                       // the last chunk has been consumed: the region becomes the triangle
    // From here on fp64.  The sums above are fp32 (the matrix cores); a factorisation and two substitutions in fp32 would add
    // several times the error those sums carry (measured: DESIGN.md, "ALS"), in fp64 they add nothing visible.
    double* A = reinterpret_cast<double*>(raw);            // A(i, j), j <= i, at i (i + 1) / 2 + j
    als_for_each<T>([&](int t, int r, int i, int j) {
        if (j <= i && i < D) {
            double v = (double)tot[t][r] + (double)p.b * (double)p.Gm[i * G::Dp + j];
            if (i == j) v += (double)p.reg;
            A[i * (i + 1) / 2 + j] = v;
            if (j == 0) lcol[0][i] = v;
        }
    });
    if (tid < G::Dp) ys[tid] = (double)ytot;
    __syncthreads();
    // Cholesky A = L L^T, column by column.  Column j stays UNSCALED in place: L(i, j) = A(i, j) dinv[j], dinv[j] = 1 / L(j, j).
    // lcol[j & 1][i] holds A(i, j) as the update of column j - 1 left it; the forward substitution L z = y rides along.
    for (int j = 0; j < D; ++j) {
        const int cur = j & 1;
        const double* lc = lcol[cur];
        const double inv = 1.0 / sqrt(lc[j]);
        const double zj = ys[j] * inv;
        if (tid == j) { dinv[j] = inv; zs[j] = zj; }
        if (tid > j && tid < D) ys[tid] = fma(-(lc[tid] * inv), zj, ys[tid]);
        // trailing update A(i, k) -= L(i, j) L(k, j), j < k <= i: 16 x 16 blocks of (i, k), thread (ti, tk) one element of each;
        // four blocks of a block row at a time, their loads ahead of their stores
        const int nb = (D - 1 - j + 15) >> 4;
        for (int a = 0; a < nb; ++a) {
            const int i = j + 1 + 16 * a + ti;
            const bool iv = i < D;
            const double li = iv ? lc[i] * inv : 0.0;
            double* Ai = A + (iv ? i * (i + 1) / 2 : 0);
            for (int b0 = 0; b0 <= a; b0 += 4) {
                double av[4], lk[4];
                bool ok[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = j + 1 + 16 * (b0 + u) + tk;
                    ok[u] = iv && b0 + u <= a && k <= i;
                    av[u] = ok[u] ? Ai[k] : 0.0;
                    lk[u] = ok[u] ? lc[k] * inv : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = j + 1 + 16 * (b0 + u) + tk;
                    if (ok[u]) {
                        const double v = fma(-li, lk[u], av[u]);
                        Ai[k] = v;
                        if (k == j + 1) lcol[cur ^ 1][i] = v;
                    }
                }
            }
        }
        __syncthreads();
    }
    // L^T x = z from the last column up: x_j = z_j dinv[j], then z_k -= L(j, k) x_j for k < j (row j of the triangle is contiguous)
    for (int j = D - 1; j > 0; --j) {
        const double xj = zs[j] * dinv[j];
        if (tid < j) zs[tid] = fma(-(A[j * (j + 1) / 2 + tid] * dinv[tid]), xj, zs[tid]);
        __syncthreads();
    }
    if (tid < D) x[tid] = (float)(zs[tid] * dinv[tid]);    // rounded to fp32 once
}

// ---------------------------------------------------------------------------------------- launchers ---
// fn(std::integral_constant<int, T>) for T = ceil(D / 16)
template <class Fn>
static int als_dispatch(int D, Fn fn) {
    switch ((D + 15) / 16) {
        case 1: return fn(std::integral_constant<int, 1>{});
        case 2: return fn(std::integral_constant<int, 2>{});
        case 3: return fn(std::integral_constant<int, 3>{});
        case 4: return fn(std::integral_constant<int, 4>{});
        case 5: return fn(std::integral_constant<int, 5>{});
        case 6: return fn(std::integral_constant<int, 6>{});
        case 7: return fn(std::integral_constant<int, 7>{});
        case 8: return fn(std::integral_constant<int, 8>{});
    }
    orx_set_error("ALS: dim %d outside [1, 128]", D);
    return ORX_ERR_ARG;
}

template <int T>
static int als_launch_T(orx_ctx* ctx, const AlsArgs& p) {
    if (p.plan.seg_base) {
        const int grid = p.plan.cap < 2048 ? p.plan.cap : 2048;
        ORX_LAUNCH(ctx, als_segment_kernel<T>, dim3(grid), dim3(ALS_THREADS), 0, p);
    }
    ORX_LAUNCH(ctx, als_solve_kernel<T>, dim3((unsigned)p.nrows), dim3(ALS_THREADS), 0, p);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

int orx_launch_als(orx_ctx* ctx, const float* F, int64_t M, int D, float* X, const int64_t* rp, const int32_t* cols, const float* conf,
                   int64_t nrows, float a, float b, float reg, const float* Gm, const SegScratch& s) {
    AlsArgs p;
    p.F = F; p.M = M; p.D = D; p.Gm = Gm; p.X = X; p.rp = rp; p.cols = cols; p.conf = conf; p.nrows = nrows;
    p.a = a; p.b = b; p.reg = reg; p.err = ctx->d_err;
    CHECK(seg_plan_launch<ALS_SEG>(ctx, rp, nrows, s, &p.plan));
    return als_dispatch(D, [&](auto t) { return als_launch_T<decltype(t)::value>(ctx, p); });
}

// the gram: Gm NULL leaves the slab partials unreduced
template <int T>
static int als_gram_T(orx_ctx* ctx, const float* F, int64_t M, int D, float* gram_part, float* Gm) {
    using G = AlsGeom<T>;
    const int nb = orx_als_gram_blocks(M);
    ORX_LAUNCH(ctx, als_gram_kernel<T>, dim3(nb), dim3(ALS_THREADS), 0, F, M, D, gram_part);
    if (Gm) ORX_LAUNCH(ctx, als_gram_reduce_kernel, dim3((G::Dp * G::Dp + 255) / 256), dim3(256), 0, (const float*)gram_part, nb, G::Dp, Gm);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

int orx_launch_als_gram(orx_ctx* ctx, const float* F, int64_t M, int D, float* gram_part, float* Gm) {
    return als_dispatch(D, [&](auto t) { return als_gram_T<decltype(t)::value>(ctx, F, M, D, gram_part, Gm); });
}
