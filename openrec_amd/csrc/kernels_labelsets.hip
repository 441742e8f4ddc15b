// The full softmax over all items with a label SET per sample (orx_seqrec_full_sets_step / orx_tower_sets_step and their
// forwards, include/openrec_hip.h has the semantics): the multinomial likelihood of Mult-DAE / Mult-VAE,
//
//   l_i = T_i lse_i - sum_e t_e s_{i,j_e} = sum_e t_e ((m_i - s_{i,j_e}) + log E_i)        e over [ptr[i], ptr[i + 1]),  T_i = sum_e t_e
//
// The gradient a_ij = c_i (T_i pi_ij - sum_{e: j_e = j} t_e) has a DENSE part over all items and a SPARSE part on the labels.
// The dense part is the three walks of kernels_fullsoftmax.hip as they are, on rows whose key (ORX_LS_KEY) no walked item
// equals: the LSE pass then sums every item into E_i, and the gradient walks take c_i T_i / E_i where the single-label form has
// c_i / tot_i, with a label coefficient that no pair ever takes.  The sparse part is here, five kernels, none of which writes a table:
//   ls_prepare_kernel   fs_prepare_kernel with the label id replaced by a walk over the set: the query row into xq, the bounds
//                       of the set and of every id in it (64 ids per coalesced load), the owner of every list position, key,
//                       c = w / B and the query side's squares.  One wavefront per sample.
//   ls_rows_kernel      after the LSE pass.  One wavefront per sample: the item chunks' (m, E) in chunk order as fs_finalize_kernel
//                       merges them, then the set 64 ids per load, four item rows in flight: s_{i,j_e} by a wave-wide dot with
//                       the row of xq (lane l holds columns l + 64 k), t_e ((m - s) + log E) added in list order, T_i,
//                       p_i = sum_e t_e V[j_e] and the entries' |V|^2.  -> m_i, c_i T_i / E_i, l_i, c_i p_i.
//   ls_reduce_kernel    one (loss, l2) partial per 256 samples, the geometry of fs_finalize_kernel.
//   ls_query_kernel     g_q[i] = scale (the chunks' partials in chunk order - c_i p_i) + the l2 term, over the rows
//                       fs_finish_kernel<0> has written: the labels' part comes off before the scale, one rounding.
//   ls_items_kernel     on the label entries sorted by item (kernels_rowsort.hip: stable, so a run is in position order, which
//                       is sample order): the wavefront at the head of a run of equal items walks the run 64 entries per load --
//                       each lane fetches its entry's owner, liveness and c_i t_e --, four query rows in flight, and subtracts
//                       the sums c_i t_e q_i and c_i t_e (Kahan: a run is up to B entries) from the sample chunks' partials of
//                       G_V[j] and G_b[j] before the scale, adds l2 n_j V[j]; the other wavefronts leave at once.  An item every
//                       sample labels is one wavefront's B entries in order.
// Every sum has a fixed order that depends on the lists and the shapes alone.  No atomics.
#include "orx_device.h"

namespace {

constexpr float LS_NEG = -3.0e38f;
constexpr int LS_UN = 4;           // row loads in flight per wavefront

// kernels_fullsoftmax.hip fs_exp, restated: the chunks are merged with the exp that made them
__device__ __forceinline__ float ls_exp(float x) {
    x = fmaxf(x, -104.0f);
    const float hi = 1.44269502162933349609375f, lo = 1.92596299e-8f;
    const float t = x * hi;
    const float r = fmaf(x, lo, fmaf(x, hi, -t));
    const float e = __builtin_amdgcn_exp2f(t);
    return fmaf(e, r * 0.693147182f, e);
}

// s += x with the rounding error of the sum carried in c (Kahan): the sums over a set of 130 entries, or over the B entries of an item
// every sample labels, stay within an ulp of their value -- they are SUBTRACTED from the dense part of a gradient
__device__ __forceinline__ void ls_add(float& s, float& c, float x) {
    const float y = x - c, t = s + y;
    c = (t - s) - y;
    s = t;
}

__global__ __launch_bounds__(256) void ls_prepare_kernel(LabelSetArgs la) {
    const FullSoftmaxArgs& a = la.fs;
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= a.Bp) return;
    const bool live = t < a.B;
    const int u = live ? a.qid[t] : 0;
    bool bad = false;
    if (live) {
        const int64_t lo = la.ptr[t], hi = la.ptr[t + 1];
        bad = lo < 0 || hi < lo || hi > la.n || (t == 0 && lo != 0) || (t == a.B - 1 && hi != la.n);
        const int64_t len = bad ? 0 : hi - lo;
        for (int64_t c0 = 0; c0 < len; c0 += 64)
            if (c0 + lane < len) {
                const int64_t e = lo + c0 + lane;
                if (!id_ok(la.items[e], a.NI)) bad = true;
                if (la.owner) la.owner[e] = (int32_t)t;
            }
    }
    const bool ok = live && id_ok(u, a.NQ) && __ballot(bad) == 0ull;
    if (live && !ok && lane == 0) *a.err = 1;
    const float* ur = a.Q + (size_t)(ok ? u : 0) * a.D;
    float sq = 0.0f;
    const int cend = a.X0 && a.x0w > a.Dp ? a.x0w : a.Dp;
    for (int c = lane; c < cend; c += 64) {
        const float x = (ok && c < a.D) ? ur[c] : 0.0f;
        if (c < a.Dp) a.xq[(size_t)t * a.Dp + c] = x;
        const float xs = a.X0 ? ((ok && c < a.x0w) ? a.X0[(size_t)t * a.x0ld + c] : 0.0f) : x;
        sq = fmaf(xs, xs, sq);
    }
    sq = wave_sum(sq);
    if (lane == 0) {
        a.key[t] = ok ? ORX_LS_KEY : -1;
        a.cw[t] = ok ? (a.wt ? a.wt[t] : 1.0f) * a.invB : 0.0f;
        a.sq[t] = sq;
    }
}

__global__ __launch_bounds__(256) void ls_rows_kernel(LabelSetArgs la) {
    const FullSoftmaxArgs& a = la.fs;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.Bp) return;
    float p[4] = {0.f, 0.f, 0.f, 0.f}, pc[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.key[i] < 0) {
        if (lane == 0) { a.rmax[i] = INFINITY; a.cn[i] = 0.0f; a.dcoef[i] = 0.0f; a.rowloss[i] = 0.0f; }
        if (la.lp && i < a.B)
            for (int k = 0; k < 4; ++k)
                if (lane + 64 * k < a.D) la.lp[(size_t)i * a.D + lane + 64 * k] = 0.0f;
        return;
    }
    float M = LS_NEG;
    for (int ch = 0; ch < a.nci; ++ch) M = fmaxf(M, a.pm[(size_t)ch * a.Bp + i]);
    float E = 0.0f;
    for (int ch = 0; ch < a.nci; ++ch) E = fmaf(a.pe[(size_t)ch * a.Bp + i], ls_exp(a.pm[(size_t)ch * a.Bp + i] - M), E);
    const float logE = logf(E);
    float xq[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) xq[k] = lane + 64 * k < a.D ? a.xq[(size_t)i * a.Dp + lane + 64 * k] : 0.0f;
    const int64_t lo = la.ptr[i], len = la.ptr[i + 1] - lo;          // (checked by ls_prepare_kernel: the sample is live)
    float lsum = 0.0f, lc = 0.0f, T = 0.0f, Tc = 0.0f, vs = 0.0f;
    for (int64_t c0 = 0; c0 < len; c0 += 64) {
        const int cnt = (int)(len - c0 < 64 ? len - c0 : 64);
        int mine = 0;
        float myt = 0.0f;
        if (lane < cnt) { mine = la.items[lo + c0 + lane]; myt = la.tw ? la.tw[lo + c0 + lane] : 1.0f; }
        for (int j0 = 0; j0 < cnt; j0 += LS_UN) {
            float v[LS_UN][4], bj[LS_UN], oj[LS_UN], tt[LS_UN];
#pragma unroll
            for (int u = 0; u < LS_UN; ++u) {
                const int id = __shfl(mine, (j0 + u) & 63);
                tt[u] = __shfl(myt, (j0 + u) & 63);
                const bool on = j0 + u < cnt;
#pragma unroll
                for (int k = 0; k < 4; ++k) v[u][k] = (on && lane + 64 * k < a.D) ? a.V[(size_t)id * a.D + lane + 64 * k] : 0.0f;
                bj[u] = on ? a.ib[id] : 0.0f;
                oj[u] = on ? a.io[id] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < LS_UN; ++u)
                if (j0 + u < cnt) {
                    float d = 0.0f;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        d = fmaf(xq[k], v[u][k], d);
                        ls_add(p[k], pc[k], tt[u] * v[u][k]);
                        vs = fmaf(v[u][k], v[u][k], vs);
                    }
                    d = wave_sum(d);
                    const float s = fmaf(a.scale, d + bj[u], oj[u]);
                    ls_add(lsum, lc, tt[u] * ((M - s) + logE));
                    ls_add(T, Tc, tt[u]);
                }
        }
    }
    vs = wave_sum(vs);
    const float c = a.cw[i];
    if (lane == 0) {
        a.rmax[i] = M;
        a.cn[i] = (c * T) / E;                 // the walks' c_i / tot_i: every item is in E, the labels among them
        a.dcoef[i] = 0.0f;                     // (no pair is a label pair)
        a.rowloss[i] = lsum;
        a.sq[i] += vs;
    }
    if (la.lp && i < a.B)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (lane + 64 * k < a.D) la.lp[(size_t)i * a.D + lane + 64 * k] = c * p[k];
}

// one thread per sample, one (loss, l2) partial per workgroup
__global__ __launch_bounds__(256) void ls_reduce_kernel(LabelSetArgs la) {
    const FullSoftmaxArgs& a = la.fs;
    __shared__ float s_l[4], s_q[4];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float cl = 0.0f, sq = 0.0f;
    if (i < a.Bp && a.key[i] >= 0) { cl = a.cw[i] * a.rowloss[i]; sq = a.sq[i]; }
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

// one thread per element of g_q: fs_finish_kernel<0>'s sum of the chunks' partials in chunk order, the labels' part taken off BEFORE
// the scale and the l2 term -- one rounding of the difference, one of the result
__global__ __launch_bounds__(256) void ls_query_kernel(LabelSetArgs la) {
    const FullSoftmaxArgs& a = la.fs;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.B * a.D) return;
    const int64_t i = idx / a.D;
    const int d = (int)(idx - i * a.D);
    float s = 0.0f;
    for (int ch = 0; ch < a.nci; ++ch) s += a.gpq[((size_t)ch * a.Bp + i) * a.Dp + d];
    a.gu[(size_t)i * a.gs + d] = fmaf(a.scale, s - la.lp[idx], a.l2q * a.xq[(size_t)i * a.Dp + d]);
}

// one wavefront per sorted position; the one at the head of a run does the run
__global__ __launch_bounds__(256) void ls_items_kernel(LabelSetArgs la, const uint2* __restrict__ sorted) {
    const FullSoftmaxArgs& a = la.fs;
    const int lane = threadIdx.x & 63;
    const int64_t k0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k0 >= la.n) return;
    const uint32_t j = sorted[k0].x;
    if (j >= (uint64_t)a.NI) return;                                    // (the sort's key of an id outside the table)
    if (k0 > 0 && sorted[k0 - 1].x == j) return;
    float sub[4] = {0.f, 0.f, 0.f, 0.f}, sc[4] = {0.f, 0.f, 0.f, 0.f};
    float bs = 0.0f, bc = 0.0f;
    int nn = 0;
    for (int64_t c0 = k0; c0 < la.n; c0 += 64) {
        const int64_t e = c0 + lane;
        uint2 pr = make_uint2(0xffffffffu, 0u);
        if (e < la.n) pr = sorted[e];
        const bool match = pr.x == j;
        const int cnt = __popcll(__ballot(match));                      // (sorted: the matches are the leading lanes)
        int ii = 0;
        float co = 0.0f;
        bool lv = false;
        if (match && pr.y < (uint64_t)la.n) {
            const int o = la.owner[pr.y];
            lv = (uint32_t)o < (uint64_t)a.B && a.key[o] >= 0;
            if (lv) { ii = o; co = a.cw[o] * (la.tw ? la.tw[pr.y] : 1.0f); }
        }
        for (int j0 = 0; j0 < cnt; j0 += LS_UN) {
            float x[LS_UN][4], cu[LS_UN];
            bool on[LS_UN];
#pragma unroll
            for (int u = 0; u < LS_UN; ++u) {
                const int r = __shfl(ii, (j0 + u) & 63);
                cu[u] = __shfl(co, (j0 + u) & 63);
                on[u] = j0 + u < cnt && __shfl((int)lv, (j0 + u) & 63) != 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) x[u][k] = (on[u] && lane + 64 * k < a.D) ? a.xq[(size_t)r * a.Dp + lane + 64 * k] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < LS_UN; ++u)
                if (on[u]) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) ls_add(sub[k], sc[k], cu[u] * x[u][k]);
                    ls_add(bs, bc, cu[u]);
                    nn += 1;
                }
        }
        if (cnt < 64) break;
    }
    // fs_finish_kernel<1>'s sums of the sample chunks' partials in chunk order, the run's part taken off BEFORE the scale and the l2 term
    const float l2n = a.l2w * (float)nn;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (lane + 64 * k < a.D) {
            const int d = lane + 64 * k;
            float s = 0.0f;
            for (int ch = 0; ch < a.ncs; ++ch) s += a.gpv[((size_t)ch * a.NIp + j) * a.Dp + d];
            a.GV[(size_t)j * a.D + d] = fmaf(a.scale, s - sub[k], l2n * a.xv[(size_t)j * a.Dp + d]);
        }
    if (lane == 0) {
        float s = 0.0f;
        for (int ch = 0; ch < a.ncs; ++ch) s += a.bpart[(size_t)ch * a.NIp + j];
        a.Gb[j] = a.scale * (s - bs);
    }
}

}  // namespace

int orx_launch_labelsets_forward(orx_ctx* ctx, const LabelSetArgs& la) {
    const FullSoftmaxArgs& a = la.fs;
    {
        ProfScope ps(ctx, ORX_K_FUSED);
        if (la.owner && la.n) ORX_HIP(hipMemsetAsync(la.owner, 0xff, (size_t)la.n * sizeof(int32_t), ctx->stream));
        ORX_LAUNCH(ctx, ls_prepare_kernel, dim3((unsigned)((a.Bp + 3) / 4)), dim3(256), 0, la);
        ORX_HIP(hipGetLastError());
    }
    CHECK(orx_launch_fullsoftmax_lse(ctx, a));
    ProfScope ps(ctx, ORX_K_FUSED);
    ORX_LAUNCH(ctx, ls_rows_kernel, dim3((unsigned)((a.Bp + 3) / 4)), dim3(256), 0, la);
    ORX_LAUNCH(ctx, ls_reduce_kernel, dim3((unsigned)orx_fullsoftmax_npartials(a.B)), dim3(256), 0, la);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

int orx_launch_labelsets_grads(orx_ctx* ctx, const LabelSetArgs& la, bool query_side, bool item_side) {
    const FullSoftmaxArgs& a = la.fs;
    CHECK(orx_launch_fullsoftmax_grads(ctx, a, query_side, item_side));
    if (query_side) {
        ProfScope ps(ctx, ORX_K_FUSED);
        ORX_LAUNCH(ctx, ls_query_kernel, dim3((unsigned)((a.B * a.D + 255) / 256)), dim3(256), 0, la);
        ORX_HIP(hipGetLastError());
    }
    if (item_side && la.n > 0) {
        const uint2* sorted = nullptr;
        CHECK(orx_rows_sort(ctx, la.items, 1, la.n, la.n, a.NI, &sorted));
        ProfScope ps(ctx, ORX_K_DUPAPPLY);
        ORX_LAUNCH(ctx, ls_items_kernel, dim3((unsigned)((la.n + 3) / 4)), dim3(256), 0, la, sorted);
        ORX_HIP(hipGetLastError());
    }
    return ORX_OK;
}
