// Dynamic negative sampling on the device (orx_sampler_pairwise_hard): every triplet's negative is the hardest of M uniform
// candidates under the current model.
//
// Stream.  Sample g = first + i takes (u, p) through smp_rec, as sample_pairwise_kernel does for (seed, g), and candidate c in
// [0, M) through smp_draw<PROP>(a, g, c, u) (orx_sampler_device.h has the formula): a uniform item, re-drawn while it is a positive
// of u.  Candidate c depends on (seed, g, c) only -- never on M, n, first or the launch shape -- and candidate 0 is the negative
// orx_sampler_pairwise writes for (seed, g), the same call.  Candidates of one sample are independent draws and may repeat.
// With a proposal (SamplerArgs::prop, the PROP = true instantiations) the draw costs one more dependent 8-byte load per attempt
// of phase B, in front of the CSR search; phases A, C and D do not know about it.
//
// Score, fp32, the kinds of orx_score_all_items: BPR U[u].V[c] + b[c], UCML -||U[u] - V[c]||^2 + b[c] (no "+ b" without a bias
// table).  Summation order: a lane adds its four products as (x0 + x1) + (x2 + x3), the lanes of a row are added by a butterfly
// (xor 1, 2, 4, ...), the bias comes last.  nid[i] is the candidate with the largest score; equal scores: the smallest c; a NaN never
// wins against a number; all NaN: candidate 0.  The selection reads the kernel's own fp32 scores, there are no atomics: a repeated
// call gives the same bits.
//
// Shape.  The work is a random gather of M item rows (and one user row) of 4 D bytes per sample.  A wavefront owns a chunk of S
// consecutive samples, S * M <= 128 slots (sample, candidate), and walks it in four phases over wavefront-private LDS:
//   A  lane j draws (u, p) of sample j
//   B  lane f draws candidate f % M of sample f / M (rejection loop and binary search per lane), into LDS and, coalesced, cand_out
//   C  LPR = D / 4 lanes (rounded up to a power of two) cover a row with one 16-byte load each, so 64 / LPR groups score as many
//      slots at once (four at D = 64); a group takes a run of consecutive slots, two per round, and loads the rows of the next
//      round before it reduces this one: four rows per group in flight.  A slot's user row stays in registers while the sample stays
//      the same.  The reduction is DPP inside 16 lanes, shuffles beyond
//   D  lane j takes the arg-max of sample j's M scores; the scores go out coalesced
// D % 4 != 0 or D > 256: the plain path, the whole wavefront on one slot with scalar loads.
#include "orx_sampler_device.h"

constexpr int HN_SLOTS = 128;       // slots (sample, candidate) of one wavefront's chunk; a chunk holds at most 64 samples

__device__ __forceinline__ float hn_partial(int ucml, f4 u, f4 v) {
    if (ucml) { const f4 d = u - v; return (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w); }
    return (u.x * v.x + u.y * v.y) + (u.z * v.z + u.w * v.w);
}

template <int LPR, bool VEC, bool PROP>
__global__ __launch_bounds__(256) void hardneg_kernel(HardNegArgs h, int S) {
    __shared__ int s_user[4][64];
    __shared__ int s_cand[4][HN_SLOTS];
    __shared__ float s_score[4][HN_SLOTS];
    const SamplerArgs& a = h.s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int M = h.M, D = h.D, ucml = h.model == ORX_UCML;
    int* su = s_user[wave]; int* sc = s_cand[wave]; float* ss = s_score[wave];
    const int64_t nchunks = (a.n + S - 1) / S;
    // (every wavefront of a workgroup takes the same number of trips: the barriers below are workgroup barriers)
    for (int64_t chunk0 = (int64_t)blockIdx.x * 4; chunk0 < nchunks; chunk0 += (int64_t)gridDim.x * 4) {
        const int64_t i0 = (chunk0 + wave) * S;
        const int ns = i0 >= a.n ? 0 : (int)(a.n - i0 < S ? a.n - i0 : S);      // samples of this wavefront's chunk
        const int nslots = ns * M;
        // ---- A: (u, p) of sample i0 + lane
        if (lane < ns) {
            const uint64_t g = (uint64_t)(a.first + i0 + lane);
            const uint64_t rec = smp_rec(a, g);
            const int u = a.rec_user[rec];
            su[lane] = u; a.uid[i0 + lane] = u; a.pid[i0 + lane] = a.rec_item[rec];
        }
        __syncthreads();
        // ---- B: the candidates
        for (int f = lane; f < nslots; f += 64) {
            const int smp = f / M, c = f - smp * M;
            const int ng = smp_draw<PROP>(a, (uint64_t)(a.first + i0 + smp), c, su[smp]);
            sc[f] = ng;
            if (h.cand) h.cand[i0 * M + f] = ng;
        }
        __syncthreads();
        // ---- C: the scores
        if (VEC) {
            constexpr int G = 64 / LPR;
            const int grp = lane / LPR, sub = lane % LPR, col = 4 * sub;
            const bool act = col < D;
            const int per = ((nslots + 2 * G - 1) / (2 * G)) * 2;       // slots of a group: an even run of consecutive ones
            const int f0 = grp * per, f1 = f0 + per < nslots ? f0 + per : nslots;
            f4 uc[2], vc[2], un[2], vn[2]; float bc[2], bn[2]; int smp_c[2], smp_n[2];
            const f4 zero = {0.f, 0.f, 0.f, 0.f};
            // the rows of slots f, f + 1; `prev` / `uprev`: the sample and user row this lane loaded last
            auto load2 = [&](int f, int prev, f4 uprev, f4 (&uu)[2], f4 (&vv)[2], float (&bb)[2], int (&sm)[2]) {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    uu[k] = uprev; vv[k] = zero; bb[k] = 0.f; sm[k] = prev;
                    if (f + k < f1) {
                        const int item = sc[f + k], smp = (f + k) / M;
                        if (act) vv[k] = *reinterpret_cast<const f4*>(h.V + (size_t)item * D + col);
                        if (h.b && sub == 0) bb[k] = h.b[item];
                        if (smp != prev) uu[k] = act ? *reinterpret_cast<const f4*>(h.U + (size_t)su[smp] * D + col) : zero;
                        sm[k] = smp; prev = smp; uprev = uu[k];
                    }
                }
            };
            load2(f0, -1, zero, uc, vc, bc, smp_c);
            for (int f = f0; f < f1; f += 2) {
                load2(f + 2, smp_c[1], uc[1], un, vn, bn, smp_n);
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const float tot = group_allreduce<LPR>(hn_partial(ucml, uc[k], vc[k]));
                    if (sub == 0 && f + k < f1) {
                        const float sv = ucml ? -tot : tot;
                        ss[f + k] = h.b ? sv + bc[k] : sv;
                    }
                }
#pragma unroll
                for (int k = 0; k < 2; ++k) { uc[k] = un[k]; vc[k] = vn[k]; bc[k] = bn[k]; smp_c[k] = smp_n[k]; }
            }
        } else {
            for (int f = 0; f < nslots; ++f) {
                const float* ur = h.U + (size_t)su[f / M] * D;
                const int item = sc[f];
                const float* vr = h.V + (size_t)item * D;
                float acc = 0.f;
                for (int d = lane; d < D; d += 64) {
                    const float x = ur[d], y = vr[d];
                    acc += ucml ? (x - y) * (x - y) : x * y;
                }
                const float tot = group_allreduce<64>(acc);
                if (lane == 0) {
                    const float sv = ucml ? -tot : tot;
                    ss[f] = h.b ? sv + h.b[item] : sv;
                }
            }
        }
        __syncthreads();
        // ---- D: the hardest candidate of sample i0 + lane
        if (lane < ns) {
            int best = 0; float sb = ss[lane * M];
            for (int c = 1; c < M; ++c) {
                const float x = ss[lane * M + c];
                if (x > sb || (sb != sb && x == x)) { sb = x; best = c; }
            }
            a.nid[i0 + lane] = sc[lane * M + best];
        }
        if (h.cand_score)
            for (int f = lane; f < nslots; f += 64) h.cand_score[i0 * M + f] = ss[f];
        __syncthreads();
    }
}

int orx_launch_hardneg(orx_ctx* ctx, const HardNegArgs& h) {
    if (h.s.n == 0) return ORX_OK;
    int S = HN_SLOTS / h.M; if (S < 1) S = 1; if (S > 64) S = 64;
    const int64_t nchunks = (h.s.n + S - 1) / S;
    int64_t g = (nchunks + 3) / 4; if (g > (int64_t)ctx->num_cu * 16) g = (int64_t)ctx->num_cu * 16;
    const dim3 grid((unsigned)g), block(256);
    const int D = h.D;
#define HN_LAUNCH(LPR, VEC)                                                                       \
    do {                                                                                          \
        if (h.s.prop) ORX_LAUNCH(ctx, (hardneg_kernel<LPR, VEC, true>), grid, block, 0, h, S);    \
        else ORX_LAUNCH(ctx, (hardneg_kernel<LPR, VEC, false>), grid, block, 0, h, S);            \
    } while (0)
    if (D % 4 != 0 || D > 256) HN_LAUNCH(64, false);
    else if (D <= 4) HN_LAUNCH(1, true);
    else if (D <= 8) HN_LAUNCH(2, true);
    else if (D <= 16) HN_LAUNCH(4, true);
    else if (D <= 32) HN_LAUNCH(8, true);
    else if (D <= 64) HN_LAUNCH(16, true);
    else if (D <= 128) HN_LAUNCH(32, true);
    else HN_LAUNCH(64, true);
#undef HN_LAUNCH
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}
