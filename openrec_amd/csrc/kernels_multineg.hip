// One positive against N sampled negatives (orx_multineg_step / orx_multineg_loss, include/openrec_hip.h has the semantics).  The
// sampler that delivers the N negatives (orx_sampler_pairwise_multi) is sample_multi_kernel of kernels_sampler.hip.
//
// multineg_grads_kernel.  One launch per step.  It reads the rows of a sample straight from the tables by id -- no gathered
// intermediate --, scores the positive and the N negatives in fp32, normalises, and writes per-occurrence gradient rows for
// orx_apply_rows: gu [B][gs]; gi [(1 + N) B][gs], the positives' rows first, then the negatives' rows in id order (sample i,
// negative j at row B + i N + j), the bias gradient in column D; the concatenated item id list [(1 + N) B] in the same order; and
// one (loss, l2) partial per wavefront.  It writes no table, so every gradient of a step is taken on the pre-step tables.
//
// Shape.  LPR = max(D / 4, 4) lanes (rounded up to a power of two) cover a row with one 16-byte load each, 64 / LPR samples run
// per wavefront, the u and p rows of a sample stay in registers across its negatives, every reduction stays inside the lane
// group (group_allreduce: DPP inside 16 lanes, shuffles beyond).  A negative is an id, then its row and bias behind the id: two
// dependent loads, so both passes fetch two negatives ahead of the one they work on (6 - 10 % of the launch's time at D = 64).
// Dims below 16 leave lanes of the group idle: they are no target, and a floor of four lanes keeps the score buffer at 16 KB
// per workgroup.
//   ORX_MN_LOGSIG   one pass: a negative's coefficient needs s_p and its own score only.
//   ORX_MN_SOFTMAX  every score before any coefficient: pass 1 leaves the N scores of a sample in wavefront-private LDS (64 floats
//                   per lane group), the group's lanes turn them into exp(s_j - m) there, each lane every LPR-th one, and sum them;
//                   pass 2 reads the negative rows again -- out of L2, a sample's rows were loaded microseconds before -- and forms
//                   the gradients.  m = max(s_p, s_0 .. s_{N-1}) is subtracted, the pi_j are summed directly for A_i (never
//                   1 - pi_p), and a sample whose positive holds the maximum takes its loss as log1p(sum_j exp(s_j - s_p)).
// D % 4 != 0 or D > 256: the plain path, the whole wavefront on one sample with scalar loads, lane j on negative j between the
// two passes.
// No atomics anywhere; the partials are added by loss_reduce_kernel in a fixed order: loss_out / l2_out are bit-repeatable.
// An id out of range raises the context's sticky index flag and is never used as an address: an invalid user or positive zeroes
// the whole sample (rows, loss and l2), an invalid negative that negative alone (it leaves the softmax as an offset of -inf would).
#include "orx_device.h"

namespace {

__device__ __forceinline__ void mn_wave_sync() {           // wavefront-private LDS: writes of some lanes, then reads of others
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// x = s_p - s_j: term = -log_sigmoid(max(x, -30)), sig = sigmoid(-x) [x >= -30] -- the expressions of score<ORX_BPR> (orx_device.h)
__device__ __forceinline__ void mn_logsig(float x, float& term, float& sig) {
    const float m = fmaxf(x, -30.0f);
    const float e = __expf(-fabsf(m));
    term = fmaxf(-m, 0.0f) + log1p_unit(e);
    const float s = (x >= 0.0f) ? e / (1.0f + e) : 1.0f / (1.0f + e);
    sig = (x >= -30.0f) ? s : 0.0f;
}

// softmax loss of a sample from s_p, the maximum m and E = sum_j exp(s_j - m); *inv_tot = 1 / sum of all 1 + N terms
__device__ __forceinline__ float mn_softmax_loss(float sp, float m, float E, float* inv_tot) {
    const float ep = __expf(sp - m);                         // (exactly 1 when the positive holds the maximum)
    const float tot = ep + E;
    *inv_tot = 1.0f / tot;
    return sp == m ? log1pf(E) : (m - sp) + logf(tot);
}

template <int LPR, int KIND, bool GRAD>
__global__ __launch_bounds__(256) void multineg_grads_kernel(MultiNegArgs a) {
    constexpr int G = 64 / LPR;
    __shared__ float s_sc[4][G * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane % LPR, grp = lane / LPR, col = 4 * sub;
    const int D = a.D, N = a.N;
    const bool act = col < D;
    const size_t gs = (size_t)a.gs;
    float* ss = s_sc[wave] + grp * 64;
    const int64_t wave_global = (int64_t)blockIdx.x * 4 + wave;
    const int64_t stride = (int64_t)gridDim.x * 4 * G;
    const f4 zero = {0.f, 0.f, 0.f, 0.f};
    const float invN = 1.0f / (float)N;
    float loss_acc = 0.0f, sq_acc = 0.0f;
    // (every lane group of a wavefront takes the same number of trips: the wavefront barriers of the softmax sit inside the loop)
    for (int64_t t0 = wave_global * G; t0 < a.B; t0 += stride) {
        const int64_t t = t0 + grp;
        const bool live = t < a.B;
        const int u = live ? a.uid[t] : 0, p = live ? a.pid[t] : 0;
        const bool ok = live && id_ok(u, a.NU) && id_ok(p, a.NI);
        if (live && !ok && sub == 0) *a.err = 1;
        const int32_t* nid = a.nid + (size_t)(live ? t : 0) * N;
        const float* off = a.off ? a.off + (size_t)(live ? t : 0) * N : nullptr;
        f4 ru = zero, rp = zero;
        float bp = 0.0f;
        if (ok && act) {
            ru = *reinterpret_cast<const f4*>(a.U + (size_t)u * D + col);
            rp = *reinterpret_cast<const f4*>(a.V + (size_t)p * D + col);
        }
        if (ok && a.b) bp = a.b[p];
        const float sp = group_allreduce<LPR>(dot4(ru, rp)) + bp;
        const float c = ok ? (a.wt ? a.wt[t] : 1.0f) * a.invB : 0.0f;
        float sq = dot4(ru, ru) + dot4(rp, rp);
        f4 acc = zero;                      // sum_j a_ij n_j
        float A = 0.0f;
        // gradient row and bias gradient of negative j, its share of g_u
        auto emit = [&](int j, float aj, f4 rn) {
            const size_t row = (size_t)a.B + (size_t)t * N + j;
            if (act) *reinterpret_cast<f4*>(a.gi + row * gs + col) = grad4(aj, ru, a.l2w, rn);
            if (sub == 0) a.gi[row * gs + D] = aj;
            acc.x = fmaf(aj, rn.x, acc.x); acc.y = fmaf(aj, rn.y, acc.y); acc.z = fmaf(aj, rn.z, acc.z); acc.w = fmaf(aj, rn.w, acc.w);
            A += aj;
        };
        // negative j: id, validity, row, bias + offset.  The loops below keep two of them in flight ahead of the one they work on
        // (an id, then the row and the bias behind it, are dependent loads)
        struct Neg { int n; bool ok; f4 r; float bo; };
        auto fetch = [&](int j) {
            Neg g; g.n = 0; g.ok = false; g.r = zero; g.bo = 0.0f;
            if (j < N && live) {
                g.n = nid[j];
                g.ok = ok && id_ok(g.n, a.NI);
                if (g.ok && act) g.r = *reinterpret_cast<const f4*>(a.V + (size_t)g.n * D + col);
                if (g.ok && a.b) g.bo = a.b[g.n];
                if (off) g.bo += off[j];
            }
            return g;
        };
        float l = 0.0f, m = sp;
        Neg g0 = fetch(0), g1 = fetch(1);
        for (int j = 0; j < N; ++j) {
            const Neg g = g0;
            g0 = g1; g1 = fetch(j + 2);
            const int n = g.n;
            const bool okj = g.ok;
            const f4 rn = g.r;
            if (live && sub == 0) {
                if (!id_ok(n, a.NI)) *a.err = 1;
                if (GRAD) a.list[(size_t)a.B + (size_t)t * N + j] = n;
            }
            float s = group_allreduce<LPR>(dot4(ru, rn)) + g.bo;
            if (!okj) s = -INFINITY;
            sq += dot4(rn, rn);
            if (KIND == ORX_MN_LOGSIG) {
                float term, sig;
                mn_logsig(sp - s, term, sig);
                l += term;
                if (GRAD && live) emit(j, okj ? c * invN * sig : 0.0f, rn);
            } else {
                if (sub == 0) ss[j] = s;
                m = fmaxf(m, s);
            }
        }
        if (KIND == ORX_MN_LOGSIG) {
            l *= invN;
        } else {
            mn_wave_sync();
            float part = 0.0f;
            for (int j = sub; j < N; j += LPR) { const float e = __expf(ss[j] - m); ss[j] = e; part += e; }
            const float E = group_allreduce<LPR>(part);
            float inv_tot;
            l = mn_softmax_loss(sp, m, E, &inv_tot);
            mn_wave_sync();
            if (GRAD && live) {
                const float ci = c * inv_tot;
                g0 = fetch(0); g1 = fetch(1);
                for (int j = 0; j < N; ++j) {
                    const Neg g = g0;
                    g0 = g1; g1 = fetch(j + 2);
                    emit(j, g.ok ? ci * ss[j] : 0.0f, g.r);
                }
            }
            mn_wave_sync();                 // (the next sample's scores overwrite ss)
        }
        if (ok) {
            sq_acc += sq;
            if (sub == 0) loss_acc += c * l;
        }
        if (GRAD && live) {
            if (act) {
                f4 gu;
                gu.x = fmaf(a.l2w, ru.x, fmaf(-A, rp.x, acc.x)); gu.y = fmaf(a.l2w, ru.y, fmaf(-A, rp.y, acc.y));
                gu.z = fmaf(a.l2w, ru.z, fmaf(-A, rp.z, acc.z)); gu.w = fmaf(a.l2w, ru.w, fmaf(-A, rp.w, acc.w));
                *reinterpret_cast<f4*>(a.gu + (size_t)t * gs + col) = gu;
                *reinterpret_cast<f4*>(a.gi + (size_t)t * gs + col) = grad4(-A, ru, a.l2w, rp);
            }
            if (sub == 0) { a.gi[(size_t)t * gs + D] = -A; a.list[t] = p; }
        }
    }
    const float ls = wave_sum(loss_acc);
    const float sqs = wave_sum(sq_acc);
    if (lane == 0) {
        float2 v; v.x = ls; v.y = 0.5f * sqs;
        *reinterpret_cast<float2*>(a.partial + 2 * wave_global) = v;
    }
}

// any dim: one wavefront per sample, lane j owns negative j between the passes
template <int KIND, bool GRAD>
__global__ __launch_bounds__(256) void multineg_grads_generic_kernel(MultiNegArgs a) {
    __shared__ float s_sc[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int D = a.D, N = a.N;
    const size_t gs = (size_t)a.gs;
    float* ss = s_sc[wave];
    const int64_t wave_global = (int64_t)blockIdx.x * 4 + wave;
    const int64_t stride = (int64_t)gridDim.x * 4;
    const float invN = 1.0f / (float)N;
    float loss_acc = 0.0f, sq_acc = 0.0f;
    for (int64_t t = wave_global; t < a.B; t += stride) {
        const int u = a.uid[t], p = a.pid[t];
        const bool ok = id_ok(u, a.NU) && id_ok(p, a.NI);          // (wave-uniform)
        if (!ok && lane == 0) *a.err = 1;
        const int32_t* nid = a.nid + (size_t)t * N;
        const float* ur = a.U + (size_t)(ok ? u : 0) * D;
        const float* pr = a.V + (size_t)(ok ? p : 0) * D;
        float part = 0.0f, sq = 0.0f;
        if (ok)
            for (int e = lane; e < D; e += 64) { const float x = ur[e], y = pr[e]; part += x * y; sq += x * x + y * y; }
        float sp = wave_sum(part);
        if (ok && a.b) sp += a.b[p];
        const float c = ok ? (a.wt ? a.wt[t] : 1.0f) * a.invB : 0.0f;
        // ---- pass 1: the scores
        float m = sp;
        for (int j = 0; j < N; ++j) {
            const int n = nid[j];
            const bool okj = ok && id_ok(n, a.NI);
            if (lane == 0) {
                if (!id_ok(n, a.NI)) *a.err = 1;
                if (GRAD) a.list[(size_t)a.B + (size_t)t * N + j] = n;
            }
            const float* nr = a.V + (size_t)(okj ? n : 0) * D;
            part = 0.0f;
            if (okj)
                for (int e = lane; e < D; e += 64) { const float y = nr[e]; part += ur[e] * y; sq += y * y; }
            float s = wave_sum(part);
            if (okj && a.b) s += a.b[n];
            if (a.off) s += a.off[(size_t)t * N + j];
            if (!okj) s = -INFINITY;
            if (lane == 0) ss[j] = s;
            m = fmaxf(m, s);
        }
        mn_wave_sync();
        // ---- the coefficients: lane j turns s_j into a_ij
        const bool mine = lane < N;
        const float sj = mine ? ss[lane] : -INFINITY;
        const bool okm = mine && ok && id_ok(nid[mine ? lane : 0], a.NI);
        float l, aj = 0.0f;
        if (KIND == ORX_MN_LOGSIG) {
            float term = 0.0f, sig = 0.0f;
            if (mine) mn_logsig(sp - sj, term, sig);
            l = wave_sum(term) * invN;
            aj = okm ? c * invN * sig : 0.0f;
        } else {
            const float e = mine ? __expf(sj - m) : 0.0f;
            const float E = wave_sum(e);
            float inv_tot;
            l = mn_softmax_loss(sp, m, E, &inv_tot);
            aj = okm ? c * inv_tot * e : 0.0f;
        }
        if (ok) {
            sq_acc += sq;
            if (lane == 0) loss_acc += c * l;
        }
        if (GRAD) {
            const float A = wave_sum(aj);
            if (mine) ss[lane] = aj;
            mn_wave_sync();
            // ---- pass 2: the gradient rows
            for (int j = 0; j < N; ++j) {
                const int n = nid[j];
                const bool okj = ok && id_ok(n, a.NI);
                const float* nr = a.V + (size_t)(okj ? n : 0) * D;
                const float cj = ss[j];
                const size_t row = (size_t)a.B + (size_t)t * N + j;
                for (int e = lane; e < D; e += 64) a.gi[row * gs + e] = okj ? fmaf(cj, ur[e], a.l2w * nr[e]) : 0.0f;
                if (lane == 0) a.gi[row * gs + D] = cj;
            }
            for (int e = lane; e < D; e += 64) {
                float accu = 0.0f;
                for (int j = 0; j < N; ++j) {
                    const int n = nid[j];
                    if (ok && id_ok(n, a.NI)) accu = fmaf(ss[j], a.V[(size_t)n * D + e], accu);
                }
                const float x = ok ? ur[e] : 0.0f, y = ok ? pr[e] : 0.0f;
                a.gu[(size_t)t * gs + e] = fmaf(a.l2w, x, fmaf(-A, y, accu));
                a.gi[(size_t)t * gs + e] = fmaf(-A, x, a.l2w * y);
            }
            if (lane == 0) { a.gi[(size_t)t * gs + D] = -A; a.list[t] = p; }
        }
        mn_wave_sync();                     // (the next sample's scores overwrite ss)
    }
    const float ls = wave_sum(loss_acc);
    const float sqs = wave_sum(sq_acc);
    if (lane == 0) {
        float2 v; v.x = ls; v.y = 0.5f * sqs;
        *reinterpret_cast<float2*>(a.partial + 2 * wave_global) = v;
    }
}

inline int mn_lpr(int D) {                  // 0: the plain path
    if (D % 4 != 0 || D > 256) return 0;
    int lpr = 4;
    while (4 * lpr < D) lpr *= 2;
    return lpr;
}

inline int64_t mn_blocks(int num_cu, int D, int64_t B) {
    const int lpr = mn_lpr(D);
    const int64_t per_wave = lpr ? 64 / lpr : 1;
    const int64_t waves = (B + per_wave - 1) / per_wave;
    int64_t g = (waves + 3) / 4;
    const int64_t cap = (int64_t)num_cu * 16;
    if (g > cap) g = cap;
    return g < 1 ? 1 : g;
}

template <int KIND, bool GRAD>
void mn_launch(orx_ctx* ctx, int lpr, dim3 g, const MultiNegArgs& a) {
    switch (lpr) {
        case 4: ORX_LAUNCH(ctx, (multineg_grads_kernel<4, KIND, GRAD>), g, dim3(256), 0, a); break;
        case 8: ORX_LAUNCH(ctx, (multineg_grads_kernel<8, KIND, GRAD>), g, dim3(256), 0, a); break;
        case 16: ORX_LAUNCH(ctx, (multineg_grads_kernel<16, KIND, GRAD>), g, dim3(256), 0, a); break;
        case 32: ORX_LAUNCH(ctx, (multineg_grads_kernel<32, KIND, GRAD>), g, dim3(256), 0, a); break;
        case 64: ORX_LAUNCH(ctx, (multineg_grads_kernel<64, KIND, GRAD>), g, dim3(256), 0, a); break;
        default: ORX_LAUNCH(ctx, (multineg_grads_generic_kernel<KIND, GRAD>), g, dim3(256), 0, a); break;
    }
}

}  // namespace

int orx_multineg_nwaves(orx_ctx* ctx, int D, int64_t B) { return (int)(mn_blocks(ctx->num_cu, D, B) * 4); }

// grads == false: the loss-only instantiations (a.gu / a.gi / a.list are not touched)
int orx_launch_multineg(orx_ctx* ctx, int kind, bool grads, const MultiNegArgs& a) {
    ProfScope ps(ctx, ORX_K_FUSED);
    const int lpr = mn_lpr(a.D);
    const dim3 g((unsigned)mn_blocks(ctx->num_cu, a.D, a.B));
    if (kind == ORX_MN_SOFTMAX) { if (grads) mn_launch<ORX_MN_SOFTMAX, true>(ctx, lpr, g, a); else mn_launch<ORX_MN_SOFTMAX, false>(ctx, lpr, g, a); }
    else { if (grads) mn_launch<ORX_MN_LOGSIG, true>(ctx, lpr, g, a); else mn_launch<ORX_MN_LOGSIG, false>(ctx, lpr, g, a); }
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}
