// Gradient kernels of the partial train step (orx_pairwise_step_subset / orx_pointwise_step_subset, api_subset.hip): a step
// that updates only the tables named by its train mask.
//
// One launch per step.  It reads the rows of a triplet (sample) straight from the tables by id -- no gathered intermediate --,
// forms the score and the gradient coefficient once, adds the step's (loss, l2_loss) partials (l2 over ALL looked-up rows,
// trained or not: bpr.py:32-36, ucml.py:30-33, wrmf.py:29-32) and writes per-occurrence gradient rows ONLY for the roles the
// mask trains (gu / gi / gb != NULL).  It writes no table: the sorted row apply of every trained table (kernels_rowsort.hip)
// runs behind it on the stream, so the gradients of a step are taken on the pre-step tables by construction, and a table
// outside the mask is only ever read.
// Users only, D = 64: 3 rows + 2 biases read, 1 row written per triplet (1.0 KB); the apply behind it moves another 0.78 KB
// (gradient row and sorted pair read, user row read and written) -- 1.82 KB against the 1.56 KB of the full step.
//
// Layout of the outputs of one step: gu [B][D]; gi [2B][D] and gb [2B] -- the gradients of the positive lookups, then those of
// the negative lookups, the order of the concatenated id list the item table's apply sorts (pointwise: [B][D] and [B]).
// A triplet with an id out of range raises the context's sticky index flag and contributes zero rows.
#include "orx_device.h"

namespace {

// WRMF.call + PointwiseMSELoss (wrmf.py:21-34, pointwise_mse_loss.py:18-31): the per-sample term and d(loss)/d(score), the
// expressions of kernels_pointwise.hip's point_score
__device__ __forceinline__ void wrmf_score(float s, float y, float a_w, float b_w, int sigmoid, float& term, float& gs) {
    const float c = (a_w - b_w) * y + b_w;
    float pred = s, dpred = 1.0f;
    if (sigmoid) {
        const float e = __expf(-fabsf(s));
        pred = (s >= 0.0f) ? 1.0f / (1.0f + e) : e / (1.0f + e);
        dpred = pred * (1.0f - pred);
    }
    const float r = y - pred;
    term = c * r * r;
    gs = -2.0f * c * r * dpred;
}

// LPR lanes own one row (D = 4 LPR), 64 / LPR triplets per wavefront per pass
// (WT: per-triplet weights SubsetArgs::wt, a compile-time variant as in fused_kernel)
template <int LPR, int MODEL, bool WT>
__global__ __launch_bounds__(256) void subset_pair_grads_kernel(SubsetArgs a) {
    constexpr int TPW = 64 / LPR;
    constexpr int D = 4 * LPR;
    constexpr bool NB = MODEL == MODEL_BPR_NB;
    constexpr int SM = NB ? (int)ORX_BPR : MODEL;
    const int lane = threadIdx.x & 63;
    const int sub = lane % LPR;
    const int grp = lane / LPR;
    const int64_t wave_global = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t stride = (int64_t)gridDim.x * 4 * TPW;
    float loss_acc = 0.0f, sq_acc = 0.0f;
    for (int64_t t = wave_global * TPW + grp; t < a.B; t += stride) {
        const int u = a.uid[t], p = a.pid[t], n = a.nid[t];
        const bool ok = id_ok(u, a.NU) & id_ok(p, a.NI) & id_ok(n, a.NI);
        f4 gu = {0.f, 0.f, 0.f, 0.f}, gp = gu, gn = gu;
        float gbp = 0.0f, gbn = 0.0f;
        if (ok) {
            const f4 ru = *reinterpret_cast<const f4*>(a.U + (size_t)u * D + 4 * sub);
            const f4 rp = *reinterpret_cast<const f4*>(a.V + (size_t)p * D + 4 * sub);
            const f4 rn = *reinterpret_cast<const f4*>(a.V + (size_t)n * D + 4 * sub);
            const float bp = NB ? 0.0f : a.b[p], bn = NB ? 0.0f : a.b[n];
            const float red = group_allreduce<LPR>(score_partial<SM>(ru, rp, rn));
            float term, g;
            if (WT) score_weighted<SM>(red, bp, bn, a.invB, a.wt[t], a.margin, term, g);
            else score<SM>(red, bp, bn, a.invB, a.margin, term, g);
            sq_acc += dot4(ru, ru) + dot4(rp, rp) + dot4(rn, rn);
            if (sub == 0) loss_acc += term;
            row_grads<SM>(ru, rp, rn, g, a.l2w, gu, gp, gn, gbp, gbn);
        } else if (sub == 0) {
            *a.err = 1;
        }
        if (a.gu) *reinterpret_cast<f4*>(a.gu + (size_t)t * D + 4 * sub) = gu;
        if (a.gi) {
            *reinterpret_cast<f4*>(a.gi + (size_t)t * D + 4 * sub) = gp;
            *reinterpret_cast<f4*>(a.gi + (size_t)(a.B + t) * D + 4 * sub) = gn;
        }
        if (!NB && a.gb && sub == 0) { a.gb[t] = gbp; a.gb[a.B + t] = gbn; }
    }
    const float ls = wave_sum(loss_acc);
    const float sq = wave_sum(sq_acc);
    if (lane == 0) {
        float2 v; v.x = ls; v.y = 0.5f * sq;
        *reinterpret_cast<float2*>(a.partial + 2 * wave_global) = v;
    }
}

// any dim: one wavefront per triplet
template <int MODEL, bool WT>
__global__ __launch_bounds__(256) void subset_pair_grads_generic_kernel(SubsetArgs a) {
    constexpr bool NB = MODEL == MODEL_BPR_NB;
    constexpr int SM = NB ? (int)ORX_BPR : MODEL;
    const int lane = threadIdx.x & 63;
    const int D = a.D;
    const int64_t wave_global = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t stride = (int64_t)gridDim.x * 4;
    float loss_acc = 0.0f, sq_acc = 0.0f;
    for (int64_t t = wave_global; t < a.B; t += stride) {
        const int u = a.uid[t], p = a.pid[t], n = a.nid[t];
        const bool ok = id_ok(u, a.NU) & id_ok(p, a.NI) & id_ok(n, a.NI);      // (wave-uniform)
        float g = 0.0f;
        const float* ur = a.U + (size_t)(ok ? u : 0) * D;
        const float* pr = a.V + (size_t)(ok ? p : 0) * D;
        const float* nr = a.V + (size_t)(ok ? n : 0) * D;
        if (ok) {
            float part = 0.0f;
            for (int e = lane; e < D; e += 64) {
                const float x = ur[e], y = pr[e], z = nr[e];
                if (SM == ORX_BPR) part += x * (y - z);
                else part += (x - z) * (x - z) - (x - y) * (x - y);
                sq_acc += x * x + y * y + z * z;
            }
            const float red = wave_sum(part);
            float term;
            if (WT) score_weighted<SM>(red, NB ? 0.0f : a.b[p], NB ? 0.0f : a.b[n], a.invB, a.wt[t], a.margin, term, g);
            else score<SM>(red, NB ? 0.0f : a.b[p], NB ? 0.0f : a.b[n], a.invB, a.margin, term, g);
            if (lane == 0) loss_acc += term;
        } else if (lane == 0) {
            *a.err = 1;
        }
        for (int e = lane; e < D; e += 64) {
            float gu = 0.0f, gp = 0.0f, gn = 0.0f;
            if (ok) {
                const float x = ur[e], y = pr[e], z = nr[e];
                if (SM == ORX_BPR) {
                    gu = g * (y - z) + a.l2w * x; gp = g * x + a.l2w * y; gn = -g * x + a.l2w * z;
                } else {
                    const float a2 = 2.0f * g;
                    gu = -a2 * (y - z) + a.l2w * x; gp = -a2 * (x - y) + a.l2w * y; gn = a2 * (x - z) + a.l2w * z;
                }
            }
            if (a.gu) a.gu[(size_t)t * D + e] = gu;
            if (a.gi) { a.gi[(size_t)t * D + e] = gp; a.gi[(size_t)(a.B + t) * D + e] = gn; }
        }
        if (!NB && a.gb && lane == 0) {
            const float gbp = ok ? (SM == ORX_BPR ? g : -g) : 0.0f;
            a.gb[t] = gbp; a.gb[a.B + t] = -gbp;
        }
    }
    const float ls = wave_sum(loss_acc);
    const float sq = wave_sum(sq_acc);
    if (lane == 0) {
        float2 v; v.x = ls; v.y = 0.5f * sq;
        *reinterpret_cast<float2*>(a.partial + 2 * wave_global) = v;
    }
}

// WRMF: sample (user, item, label); pid holds the item ids
template <int LPR>
__global__ __launch_bounds__(256) void subset_point_grads_kernel(SubsetArgs a) {
    constexpr int TPW = 64 / LPR;
    constexpr int D = 4 * LPR;
    const int lane = threadIdx.x & 63;
    const int sub = lane % LPR;
    const int grp = lane / LPR;
    const int64_t wave_global = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t stride = (int64_t)gridDim.x * 4 * TPW;
    float loss_acc = 0.0f, sq_acc = 0.0f;
    for (int64_t t = wave_global * TPW + grp; t < a.B; t += stride) {
        const int u = a.uid[t], i = a.pid[t];
        const bool ok = id_ok(u, a.NU) & id_ok(i, a.NI);
        f4 gu = {0.f, 0.f, 0.f, 0.f}, gi = gu;
        float gs = 0.0f;
        if (ok) {
            const f4 ru = *reinterpret_cast<const f4*>(a.U + (size_t)u * D + 4 * sub);
            const f4 ri = *reinterpret_cast<const f4*>(a.V + (size_t)i * D + 4 * sub);
            const float s = group_allreduce<LPR>(dot4(ru, ri)) + a.b[i];
            float term;
            wrmf_score(s, a.label[t], a.a_w, a.b_w, a.sigmoid, term, gs);
            sq_acc += dot4(ru, ru) + dot4(ri, ri);
            if (sub == 0) loss_acc += term;
            gu = gs * ri + a.l2w * ru;
            gi = gs * ru + a.l2w * ri;
        } else if (sub == 0) {
            *a.err = 1;
        }
        if (a.gu) *reinterpret_cast<f4*>(a.gu + (size_t)t * D + 4 * sub) = gu;
        if (a.gi) *reinterpret_cast<f4*>(a.gi + (size_t)t * D + 4 * sub) = gi;
        if (a.gb && sub == 0) a.gb[t] = gs;
    }
    const float ls = wave_sum(loss_acc);
    const float sq = wave_sum(sq_acc);
    if (lane == 0) {
        float2 v; v.x = ls; v.y = 0.5f * sq;
        *reinterpret_cast<float2*>(a.partial + 2 * wave_global) = v;
    }
}

__global__ __launch_bounds__(256) void subset_point_grads_generic_kernel(SubsetArgs a) {
    const int lane = threadIdx.x & 63;
    const int D = a.D;
    const int64_t wave_global = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t stride = (int64_t)gridDim.x * 4;
    float loss_acc = 0.0f, sq_acc = 0.0f;
    for (int64_t t = wave_global; t < a.B; t += stride) {
        const int u = a.uid[t], i = a.pid[t];
        const bool ok = id_ok(u, a.NU) & id_ok(i, a.NI);
        const float* ur = a.U + (size_t)(ok ? u : 0) * D;
        const float* ir = a.V + (size_t)(ok ? i : 0) * D;
        float gs = 0.0f;
        if (ok) {
            float part = 0.0f;
            for (int e = lane; e < D; e += 64) {
                const float x = ur[e], z = ir[e];
                part += x * z;
                sq_acc += x * x + z * z;
            }
            const float s = wave_sum(part) + a.b[i];
            float term;
            wrmf_score(s, a.label[t], a.a_w, a.b_w, a.sigmoid, term, gs);
            if (lane == 0) loss_acc += term;
        } else if (lane == 0) {
            *a.err = 1;
        }
        for (int e = lane; e < D; e += 64) {
            const float x = ok ? ur[e] : 0.0f, z = ok ? ir[e] : 0.0f;
            if (a.gu) a.gu[(size_t)t * D + e] = gs * z + a.l2w * x;
            if (a.gi) a.gi[(size_t)t * D + e] = gs * x + a.l2w * z;
        }
        if (a.gb && lane == 0) a.gb[t] = gs;
    }
    const float ls = wave_sum(loss_acc);
    const float sq = wave_sum(sq_acc);
    if (lane == 0) {
        float2 v; v.x = ls; v.y = 0.5f * sq;
        *reinterpret_cast<float2*>(a.partial + 2 * wave_global) = v;
    }
}

// ids of the item table's apply, all K steps in one launch: out [K][2B] = step k's positive ids, then its negative ids
__global__ __launch_bounds__(256) void subset_concat_ids_kernel(const int32_t* pid, const int32_t* nid, int64_t id_stride, int64_t B, int32_t* out) {
    const int64_t k = blockIdx.y;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < B; i += (int64_t)gridDim.x * 256) {
        out[k * 2 * B + i] = pid[k * id_stride + i];
        out[k * 2 * B + B + i] = nid[k * id_stride + i];
    }
}

inline int lpr_of(int D) {
    switch (D) { case 16: return 4; case 32: return 8; case 64: return 16; case 128: return 32; case 256: return 64; default: return 0; }
}

template <int MODEL, bool WT>
void launch_pair(orx_ctx* ctx, int lpr, dim3 g, const SubsetArgs& a) {
    switch (lpr) {
        case 4: ORX_LAUNCH(ctx, (subset_pair_grads_kernel<4, MODEL, WT>), g, dim3(256), 0, a); break;
        case 8: ORX_LAUNCH(ctx, (subset_pair_grads_kernel<8, MODEL, WT>), g, dim3(256), 0, a); break;
        case 16: ORX_LAUNCH(ctx, (subset_pair_grads_kernel<16, MODEL, WT>), g, dim3(256), 0, a); break;
        case 32: ORX_LAUNCH(ctx, (subset_pair_grads_kernel<32, MODEL, WT>), g, dim3(256), 0, a); break;
        case 64: ORX_LAUNCH(ctx, (subset_pair_grads_kernel<64, MODEL, WT>), g, dim3(256), 0, a); break;
        default: ORX_LAUNCH(ctx, (subset_pair_grads_generic_kernel<MODEL, WT>), g, dim3(256), 0, a); break;
    }
}

}  // namespace

// model: ORX_BPR / ORX_UCML / MODEL_BPR_NB, or < 0 for WRMF.  The step's partials go to a.partial [orx_fused_nwaves(D, B)][2].
int orx_launch_subset_grads(orx_ctx* ctx, int model, const SubsetArgs& a) {
    ProfScope ps(ctx, model < 0 ? ORX_K_POINT : ORX_K_FUSED);
    const int lpr = lpr_of(a.D);
    const dim3 g((unsigned)(orx_fused_nwaves(a.D, a.B) / 4));
    if (model >= 0 && a.wt != nullptr) {
        if (model == ORX_BPR) launch_pair<ORX_BPR, true>(ctx, lpr, g, a);
        else if (model == ORX_UCML) launch_pair<ORX_UCML, true>(ctx, lpr, g, a);
        else launch_pair<MODEL_BPR_NB, true>(ctx, lpr, g, a);
    } else if (model == ORX_BPR) launch_pair<ORX_BPR, false>(ctx, lpr, g, a);
    else if (model == ORX_UCML) launch_pair<ORX_UCML, false>(ctx, lpr, g, a);
    else if (model == MODEL_BPR_NB) launch_pair<MODEL_BPR_NB, false>(ctx, lpr, g, a);
    else {
        switch (lpr) {
            case 4: ORX_LAUNCH(ctx, subset_point_grads_kernel<4>, g, dim3(256), 0, a); break;
            case 8: ORX_LAUNCH(ctx, subset_point_grads_kernel<8>, g, dim3(256), 0, a); break;
            case 16: ORX_LAUNCH(ctx, subset_point_grads_kernel<16>, g, dim3(256), 0, a); break;
            case 32: ORX_LAUNCH(ctx, subset_point_grads_kernel<32>, g, dim3(256), 0, a); break;
            case 64: ORX_LAUNCH(ctx, subset_point_grads_kernel<64>, g, dim3(256), 0, a); break;
            default: ORX_LAUNCH(ctx, subset_point_grads_generic_kernel, g, dim3(256), 0, a); break;
        }
    }
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

int orx_launch_subset_concat_ids(orx_ctx* ctx, const int32_t* pid, const int32_t* nid, int64_t id_stride, int64_t K, int64_t B, int32_t* out) {
    ProfScope ps(ctx, ORX_K_DEDUP);
    ORX_LAUNCH(ctx, subset_concat_ids_kernel, dim3((unsigned)std::min<int64_t>((B + 255) / 256, 1024), (unsigned)K), dim3(256), 0, pid, nid, id_stride, B, out);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}
