// Graph propagation over a CSR (LightGCN's operator) and the dense pieces of its train step.  gfx950.
//
//   y[r]   = row_scale[r] * sum_{e in row r, CSR order} col_scale[cols[e]] * X[cols[e]]          (fp32)
//   out[r] = y[r];   acc[r] += acc_alpha * y[r]   (acc != NULL)
//
// The walk.  A neighbour row of D = 4 LPR floats is LPR lanes x float4, so a wavefront holds G = 64 / LPR neighbour rows per load
// instruction (D = 64: 4 rows of 256 B); GS_UN such instructions are in flight per wavefront, 16 or more wavefronts per CU
// (256-thread workgroups, 60 VGPRs, one wavefront per row).  Lane group g of a wavefront adds the entries g, g + G, g + 2 G, ... of its SEGMENT (below) in
// that order into its own float4; at the end of the segment the G group sums are combined by a butterfly over the lane groups
// (xor 32, 16, ... LPR), the same tree in every lane.  Other dims (any D <= 128): one neighbour row per load, lane l holds the
// columns l and l + 64, the entries are added in CSR order.
//
// Segments.  A row of n entries is cut into ceil(n / GS_SEG) segments of GS_SEG entries (the last one shorter).  Every segment is
// summed from zero by the walk above; a row's value is the segments' sums added in segment order, times row_scale.  Rows of one
// segment are summed and finished by their own wavefront.  The segments of longer rows are listed by seg_plan_kernel (one thread per
// row; an INTEGER counter hands out scratch slots, so slot numbers depend on the launch but nothing written into a slot does),
// summed by separate wavefronts into the slots, and added in segment order by the row's wavefront.  A row that found no slot
// walks its segments itself, the same sums in the same order.  So y[r] is a function of X, the row's entries and the scales
// alone, and the order of its additions a function of n and D alone; there is no float atomic and no trip count that depends on
// a float.
//
// A column outside X is dropped from its row and raises the context's index flag.
#include "orx_graph.h"
#include "orx_device.h"

namespace {

constexpr int GS_UN = 4;           // load instructions in flight per wavefront

struct SpmmArgs {
    const float* X; int64_t M; int D;              // the table the columns index
    float* out; float* acc; float acc_alpha;       // rows of the call's first row on (acc may be NULL)
    const int64_t* rp;                             // [nrows + 1] offsets of the call's rows
    const int32_t* cols;                           // entry e of the CSR is cols[e] (the pointer is already shifted for a staged copy)
    const float* rs; const float* cs;              // row scales of the call's first row on / column scales (NULL: 1)
    int64_t nrows;
    SegPlan plan;                                  // slots: [cap][D]
    int* err;
};

// LPR > 0: the float4 walk, the sum of entries [e0, e1) ends up in EVERY lane group (lane sub holds columns 4 sub .. 4 sub + 3)
template <int LPR>
__device__ __forceinline__ f4 seg_sum_vec(const SpmmArgs& p, int64_t e0, int64_t e1, int lane) {
    constexpr int G = 64 / LPR;
    const int sub = lane % LPR, grp = lane / LPR;
    f4 s = {0.f, 0.f, 0.f, 0.f};
    for (int64_t b = e0; b < e1; b += (int64_t)G * GS_UN) {
        f4 x[GS_UN]; float w[GS_UN];
#pragma unroll
        for (int u = 0; u < GS_UN; ++u) {
            const int64_t e = b + (int64_t)u * G + grp;
            x[u] = f4{0.f, 0.f, 0.f, 0.f}; w[u] = 0.f;
            if (e < e1) {
                const int32_t c = p.cols[e];
                if ((uint32_t)c < (uint64_t)p.M) {
                    w[u] = p.cs ? p.cs[c] : 1.0f;
                    x[u] = *reinterpret_cast<const f4*>(p.X + (size_t)c * p.D + 4 * sub);
                } else *p.err = 1;
            }
        }
#pragma unroll
        for (int u = 0; u < GS_UN; ++u) {
            const int64_t e = b + (int64_t)u * G + grp;
            if (e < e1) { s.x += w[u] * x[u].x; s.y += w[u] * x[u].y; s.z += w[u] * x[u].z; s.w += w[u] * x[u].w; }
        }
    }
#pragma unroll
    for (int off = 32; off >= LPR; off >>= 1) {
        s.x += __shfl_xor(s.x, off); s.y += __shfl_xor(s.y, off); s.z += __shfl_xor(s.z, off); s.w += __shfl_xor(s.w, off);
    }
    return s;
}

// any D <= 128: lane l holds columns l and l + 64
__device__ __forceinline__ void seg_sum_gen(const SpmmArgs& p, int64_t e0, int64_t e1, int lane, float& s0, float& s1) {
    s0 = 0.f; s1 = 0.f;
    const bool h0 = lane < p.D, h1 = lane + 64 < p.D;
    for (int64_t b = e0; b < e1; b += GS_UN) {
        float x0[GS_UN], x1[GS_UN], w[GS_UN];
#pragma unroll
        for (int u = 0; u < GS_UN; ++u) {
            const int64_t e = b + u;
            x0[u] = x1[u] = w[u] = 0.f;
            if (e < e1) {
                const int32_t c = p.cols[e];
                if ((uint32_t)c < (uint64_t)p.M) {
                    w[u] = p.cs ? p.cs[c] : 1.0f;
                    const float* row = p.X + (size_t)c * p.D;
                    if (h0) x0[u] = row[lane];
                    if (h1) x1[u] = row[lane + 64];
                } else *p.err = 1;
            }
        }
#pragma unroll
        for (int u = 0; u < GS_UN; ++u)
            if (b + u < e1) { s0 += w[u] * x0[u]; s1 += w[u] * x1[u]; }
    }
}

__device__ __forceinline__ int64_t seg_end(int64_t e0, int64_t r1) { return e0 + GS_SEG < r1 ? e0 + GS_SEG : r1; }

// one wavefront per listed segment: its sum, from zero, into its slot
template <int LPR>
__global__ __launch_bounds__(256) void graph_segment_kernel(SpmmArgs p) {
    const int lane = threadIdx.x & 63;
    const int count = seg_plan_count(p.plan);
    for (int it = blockIdx.x * 4 + (threadIdx.x >> 6); it < count; it += gridDim.x * 4) {
        const int2 w = p.plan.list[it];
        if (w.x < 0) continue;
        const int64_t r1 = p.rp[w.x + 1], e0 = p.rp[w.x] + (int64_t)w.y * GS_SEG, e1 = seg_end(e0, r1);
        float* slot = p.plan.slots + (size_t)it * p.D;
        if constexpr (LPR > 0) {
            const f4 s = seg_sum_vec<LPR>(p, e0, e1, lane);
            if (lane < LPR) *reinterpret_cast<f4*>(slot + 4 * lane) = s;
        } else {
            float s0, s1;
            seg_sum_gen(p, e0, e1, lane, s0, s1);
            if (lane < p.D) slot[lane] = s0;
            if (lane + 64 < p.D) slot[lane + 64] = s1;
        }
    }
}

// one wavefront per row of the call
template <int LPR>
__global__ __launch_bounds__(256) void graph_row_kernel(SpmmArgs p) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= p.nrows) return;
    const int64_t r0 = p.rp[r], r1 = p.rp[r + 1];
    const int64_t nseg = r1 > r0 ? (r1 - r0 + GS_SEG - 1) / GS_SEG : 0;
    const int base = (nseg > 1 && p.plan.seg_base != nullptr) ? p.plan.seg_base[r] : -1;
    const float scale = p.rs ? p.rs[r] : 1.0f;
    float* o = p.out + (size_t)r * p.D;
    float* a = p.acc ? p.acc + (size_t)r * p.D : nullptr;
    if constexpr (LPR > 0) {
        constexpr int L = LPR;
        f4 s = {0.f, 0.f, 0.f, 0.f};
        for (int64_t sg = 0; sg < nseg; ++sg) {
            f4 q;
            if (base >= 0) q = *reinterpret_cast<const f4*>(p.plan.slots + (size_t)(base + sg) * p.D + 4 * (lane % L));
            else { const int64_t e0 = r0 + sg * GS_SEG; q = seg_sum_vec<L>(p, e0, seg_end(e0, r1), lane); }
            if (sg == 0) s = q; else { s.x += q.x; s.y += q.y; s.z += q.z; s.w += q.w; }
        }
        if (lane < L) {
            if (nseg == 0) { *reinterpret_cast<f4*>(o + 4 * lane) = f4{0.f, 0.f, 0.f, 0.f}; return; }
            const f4 y = {scale * s.x, scale * s.y, scale * s.z, scale * s.w};
            *reinterpret_cast<f4*>(o + 4 * lane) = y;
            if (a) {
                f4 t = *reinterpret_cast<const f4*>(a + 4 * lane);
                t.x += p.acc_alpha * y.x; t.y += p.acc_alpha * y.y; t.z += p.acc_alpha * y.z; t.w += p.acc_alpha * y.w;
                *reinterpret_cast<f4*>(a + 4 * lane) = t;
            }
        }
    } else {
        float s0 = 0.f, s1 = 0.f;
        for (int64_t sg = 0; sg < nseg; ++sg) {
            float q0 = 0.f, q1 = 0.f;
            if (base >= 0) {
                const float* slot = p.plan.slots + (size_t)(base + sg) * p.D;
                if (lane < p.D) q0 = slot[lane];
                if (lane + 64 < p.D) q1 = slot[lane + 64];
            } else { const int64_t e0 = r0 + sg * GS_SEG; seg_sum_gen(p, e0, seg_end(e0, r1), lane, q0, q1); }
            if (sg == 0) { s0 = q0; s1 = q1; } else { s0 += q0; s1 += q1; }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int col = lane + 64 * h;
            if (col >= p.D) continue;
            if (nseg == 0) { o[col] = 0.f; continue; }
            const float y = scale * (h ? s1 : s0);
            o[col] = y;
            if (a) a[col] += p.acc_alpha * y;
        }
    }
}

template <int LPR>
int launch_spmm_T(orx_ctx* ctx, const SpmmArgs& p) {
    if (p.plan.seg_base) {
        const int blocks = std::max(1, std::min(ctx->num_cu * 8, (p.plan.cap + 3) / 4));
        ORX_LAUNCH(ctx, graph_segment_kernel<LPR>, dim3((unsigned)blocks), dim3(256), 0, p);
    }
    ORX_LAUNCH(ctx, graph_row_kernel<LPR>, dim3((unsigned)((p.nrows + 3) / 4)), dim3(256), 0, p);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

// ---- dense pieces -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void graph_scale_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t n, float alpha) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) out[i] = alpha * in[i];
}

// the Keras dense rule on every element; the gradient is read only
template <int KIND>
__global__ __launch_bounds__(256) void apply_dense_kernel(float* __restrict__ w, float* __restrict__ s0, float* __restrict__ s1, const float* __restrict__ g,
                                                          int64_t n, float lr, float eps, float b1, float b2) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float gi = g[i];
        if (KIND == ORX_SGD) w[i] = w[i] - lr * gi;
        else if (KIND == ORX_MOMENTUM) { float a = s0[i]; w[i] = mom_elem(w[i], gi, a, lr, eps); s0[i] = a; }
        else if (KIND == ORX_ADAGRAD) { const float a = s0[i] + gi * gi; s0[i] = a; w[i] = w[i] - lr * gi / (sqrtf(a) + eps); }
        else { float wi = w[i], m = s0[i], v = s1[i]; adam_elem(wi, m, v, gi, lr, b1, b2, eps); w[i] = wi; s0[i] = m; s1[i] = v; }
    }
}

// the l2 term of the layer-0 rows of a batch: one wavefront per occurrence k of ids (row ids[k] of W) writes coef * row into
// grads[k] and its share of the l2 loss, 0.5 coef |row|^2, into partial[2 wave + 1] (partial[2 wave] = 0)
__global__ __launch_bounds__(256) void graph_l2_rows_kernel(const float* __restrict__ W, int64_t rows, int D, const int32_t* __restrict__ ids, int64_t n,
                                                            float coef, float* __restrict__ grads, float* __restrict__ partial, int* err) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * 4;
    float sq = 0.f;
    for (int64_t k = wave; k < n; k += nw) {
        const int32_t r = ids[k];
        const bool ok = (uint32_t)r < (uint64_t)rows;
        if (!ok && lane == 0) *err = 1;
        for (int col = lane; col < D; col += 64) {
            const float x = ok ? W[(size_t)r * D + col] : 0.f;
            if (grads) grads[(size_t)k * D + col] = coef * x;
            sq += x * x;
        }
    }
    sq = wave_sum(sq);
    if (lane == 0) { partial[2 * wave] = 0.f; partial[2 * wave + 1] = 0.5f * coef * sq; }
}

__global__ void graph_concat_ids_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b, int64_t n, int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { out[i] = a[i]; out[n + i] = b[i]; }
}

inline unsigned grid_cap(int64_t n, int per) {
    int64_t g = (n + per - 1) / per;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(g, 256 * 32));
}

}  // namespace

// the whole product on the context's stream: plan + segment sums (cap > 0), then the rows.  vec_ok: every row of X, out and acc
// starts on a 16-byte boundary
int orx_launch_graph_spmm(orx_ctx* ctx, const float* X, int64_t M, int D, float* out, float* acc, float acc_alpha, const int64_t* rp,
                          const int32_t* cols, const float* rs, const float* cs, int64_t nrows, bool vec_ok, const SegScratch& s) {
    SpmmArgs p;
    p.X = X; p.M = M; p.D = D; p.out = out; p.acc = acc; p.acc_alpha = acc_alpha; p.rp = rp; p.cols = cols; p.rs = rs; p.cs = cs;
    p.nrows = nrows; p.err = ctx->d_err;
    CHECK(seg_plan_launch<GS_SEG>(ctx, rp, nrows, s, &p.plan));
    ProfScope ps(ctx, ORX_K_FUSED);
    if (vec_ok) {
        switch (D) {
            case 16: return launch_spmm_T<4>(ctx, p);
            case 32: return launch_spmm_T<8>(ctx, p);
            case 64: return launch_spmm_T<16>(ctx, p);
            case 128: return launch_spmm_T<32>(ctx, p);
        }
    }
    return launch_spmm_T<0>(ctx, p);
}

int orx_launch_graph_scale(orx_ctx* ctx, const float* in, float* out, int64_t n, float alpha) {
    if (n == 0) return ORX_OK;
    ORX_LAUNCH(ctx, graph_scale_kernel, dim3(grid_cap(n, 256)), dim3(256), 0, in, out, n, alpha);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

int orx_launch_apply_dense(orx_ctx* ctx, int kind, float* w, float* s0, float* s1, const float* g, int64_t n, float lr, float eps, float b1, float b2) {
    if (n == 0) return ORX_OK;
    ProfScope ps(ctx, ORX_K_SWEEP);
    const dim3 grid(grid_cap(n, 256));
    switch (kind) {
        case ORX_SGD: ORX_LAUNCH(ctx, apply_dense_kernel<ORX_SGD>, grid, dim3(256), 0, w, s0, s1, g, n, lr, eps, b1, b2); break;
        case ORX_MOMENTUM: ORX_LAUNCH(ctx, apply_dense_kernel<ORX_MOMENTUM>, grid, dim3(256), 0, w, s0, s1, g, n, lr, eps, b1, b2); break;
        case ORX_ADAGRAD: ORX_LAUNCH(ctx, apply_dense_kernel<ORX_ADAGRAD>, grid, dim3(256), 0, w, s0, s1, g, n, lr, eps, b1, b2); break;
        case ORX_ADAM: ORX_LAUNCH(ctx, apply_dense_kernel<ORX_ADAM>, grid, dim3(256), 0, w, s0, s1, g, n, lr, eps, b1, b2); break;
        default: orx_set_error("orx_table_apply_dense: unknown optimizer kind %d", kind); return ORX_ERR_ARG;
    }
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

int orx_graph_l2_nwaves(int64_t n) { return (int)grid_cap(n, 4) * 4; }

int orx_launch_graph_l2_rows(orx_ctx* ctx, const float* W, int64_t rows, int D, const int32_t* ids, int64_t n, float coef, float* grads, float* partial) {
    ORX_LAUNCH(ctx, graph_l2_rows_kernel, dim3(grid_cap(n, 4)), dim3(256), 0, W, rows, D, ids, n, coef, grads, partial, ctx->d_err);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

int orx_launch_graph_concat_ids(orx_ctx* ctx, const int32_t* a, const int32_t* b, int64_t n, int32_t* out) {
    if (n == 0) return ORX_OK;
    ORX_LAUNCH(ctx, graph_concat_ids_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, a, b, n, out);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}
