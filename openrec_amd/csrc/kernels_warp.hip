// WARP negatives on the device (orx_sampler_pairwise_warp): every triplet's negative is the FIRST of up to T candidates that violates
// the margin against the positive under the current model, and the triplet's weight is a table entry of the trial count.
//
// Stream.  (u, p) of sample g = first + i and candidate c of it are orx_sampler_pairwise_hard's: smp_rec and smp_draw<PROP> of
// orx_sampler_device.h (seed_c, the rejection loop against the user's CSR row, at most 256 attempts, the alias table when a
// proposal is set), the calls kernels_hardneg.hip makes.
//
// Score, fp32: BPR U[u].V[j] + b[j], UCML -||U[u] - V[j]||^2 + b[j] (no "+ b" without a bias table), for the positive (s_p) and the
// candidates (s_c) by ONE row scorer.  Summation order: a lane adds its four products as (x0 + x1) + (x2 + x3), the lanes of a row
// are added by a butterfly (xor 1, 2, 4, ...), the bias comes last.  (The plain path: lane l adds the columns l, l + 64, .. in
// order, then the butterfly over the 64 lanes, then the bias.)  Candidate c violates iff (s_c + margin) > s_p: one rounded fp32 add,
// one compare, so a NaN on either side never violates.  t = 1 + the smallest violating c < T, or 0.
//
// Shape.  The cost is data dependent: a sample stops being scored at its first violator.  A workgroup is ONE wavefront (64 threads),
// so the barriers below are wave barriers and the number of rounds may differ from wavefront to wavefront; its LDS is its own.  The
// wavefront owns a chunk of S consecutive samples, lane j keeps sample j's state in registers (open?, s_p, t, the negative), and
//   A  lane j draws (u, p) of sample j
//   P  the positives are scored as ns slots (sample j, item p_j) by the row scorer of C
//   then rounds, until no sample of the chunk is open or all T candidates are used (at most T rounds, every round takes R >= 1):
//     the open samples are compacted by a 64-bit ballot and a popcount prefix; every open sample has tried the same number of
//     candidates (`tried`, wave-uniform), and takes R = clamp(min(budget / open, r0 2^round), 1, T - tried) more, open * R <= 128
//     slots: the first round scores r0 = 2 candidates per sample and the count doubles from round to round, because most samples
//     of an untrained or half-trained model violate at once and every candidate behind a violator is a wasted row
//   B  lane f draws candidate tried + f % R of the (f / R)-th open sample (rejection loop and binary search per lane)
//   C  LPR = D / 4 lanes (rounded up to a power of two) cover a row with one 16-byte load each, 64 / LPR groups score as many slots
//      at once; a group takes a run of consecutive slots, two per trip, and loads the rows of the next trip before it reduces this
//      one.  A slot's user row stays in registers while the sample stays the same.  DPP inside 16 lanes, shuffles beyond.  All
//      lanes of a group take the same trips: nothing in the slot loop depends on a lane.
//   D  the lane of an open sample scans its R scores IN CANDIDATE ORDER for the first violator and writes that prefix of cand_score
// Because the scan is in candidate order, the result does not depend on R, S, the budget, r0 or the launch shape; candidates scored
// past a violator in the same round are the only wasted gathers.  S = 16, budget = 128, r0 = 2 are measured choices.  D % 4 != 0 or D > 256: the plain path, the whole wavefront on one slot.
#include "orx_sampler_device.h"

constexpr int WN_SLOTS = 128;       // slots (sample, item) of one round; a chunk holds at most 64 samples

__device__ __forceinline__ float wn_partial(int ucml, f4 u, f4 v) {
    if (ucml) { const f4 d = u - v; return (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w); }
    return (u.x * v.x + u.y * v.y) + (u.z * v.z + u.w * v.w);
}

// ss[f] = the score of (user su[ssmp[f]], item sitem[f]) for the slots f < nslots (nslots <= WN_SLOTS is wave-uniform).  Called by
// all 64 lanes; the caller puts a barrier in front of it and behind it.
template <int LPR, bool VEC>
__device__ __forceinline__ void wn_score(const WarpNegArgs& h, int nslots, const int* su, const int* sitem, const int* ssmp,
                                         float* ss, int lane) {
    const int D = h.D, ucml = h.model == ORX_UCML;
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
                    const int item = sitem[f + k], smp = ssmp[f + k];
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
                const float tot = group_allreduce<LPR>(wn_partial(ucml, uc[k], vc[k]));
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
            const float* ur = h.U + (size_t)su[ssmp[f]] * D;
            const int item = sitem[f];
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
}

// One wavefront per workgroup: __syncthreads() orders this wavefront's LDS traffic and nothing else waits on it.
template <int LPR, bool VEC, bool PROP>
__global__ __launch_bounds__(64) void warpneg_kernel(WarpNegArgs h, int S, int budget, int r0) {
    __shared__ int s_user[64];
    __shared__ int s_open[64];
    __shared__ int s_item[WN_SLOTS];
    __shared__ int s_smp[WN_SLOTS];
    __shared__ float s_score[WN_SLOTS];
    const SamplerArgs& a = h.s;
    const int lane = threadIdx.x;
    const int T = h.T;
    const int64_t nchunks = (a.n + S - 1) / S;
    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const int64_t i0 = chunk * S;
        const int ns = (int)(a.n - i0 < S ? a.n - i0 : S);          // samples of this chunk, 1 .. 64
        // ---- A: (u, p) of sample i0 + lane
        if (lane < ns) {
            const uint64_t g = (uint64_t)(a.first + i0 + lane);
            const uint64_t rec = smp_rec(a, g);
            const int u = a.rec_user[rec], p = a.rec_item[rec];
            s_user[lane] = u; s_item[lane] = p; s_smp[lane] = lane;
            a.uid[i0 + lane] = u; a.pid[i0 + lane] = p;
        }
        __syncthreads();
        // ---- P: the positives
        wn_score<LPR, VEC>(h, ns, s_user, s_item, s_smp, s_score, lane);
        __syncthreads();
        const float sp = lane < ns ? s_score[lane] : 0.f;
        bool open = lane < ns;
        int t = 0, neg = 0, c0 = 0, tried = 0, rcap = r0;
        // ---- rounds: at most T, every one takes R >= 1 candidates of every open sample
        for (int round = 0; round < T; ++round) {
            const unsigned long long mask = __ballot(open);
            const int nopen = __popcll(mask);
            if (nopen == 0 || tried >= T) break;                    // wave-uniform
            int R = budget / nopen;
            R = R < rcap ? R : rcap; R = R < 1 ? 1 : R; R = R < T - tried ? R : T - tried;
            rcap = rcap < 128 ? 2 * rcap : 256;
            const int k = __popcll(mask & ((1ull << lane) - 1ull)); // this sample's place among the open ones
            if (open) s_open[k] = lane;
            __syncthreads();
            const int nslots = nopen * R;                           // <= max(budget, 64) <= WN_SLOTS
            // ---- B: the candidates tried .. tried + R - 1 of the open samples
            for (int f = lane; f < nslots; f += 64) {
                const int kk = f / R, smp = s_open[kk];
                s_item[f] = smp_draw<PROP>(a, (uint64_t)(a.first + i0 + smp), tried + (f - kk * R), s_user[smp]);
                s_smp[f] = smp;
            }
            __syncthreads();
            // ---- C: their scores
            wn_score<LPR, VEC>(h, nslots, s_user, s_item, s_smp, s_score, lane);
            __syncthreads();
            // ---- D: the first violator, in candidate order
            if (open) {
                const int base = k * R;
                if (tried == 0) c0 = s_item[base];
                for (int r = 0; r < R; ++r) {
                    const float sc = s_score[base + r];
                    if (h.cand_score) h.cand_score[(i0 + lane) * T + tried + r] = sc;
                    if ((sc + h.margin) > sp) { t = tried + r + 1; neg = s_item[base + r]; open = false; break; }
                }
            }
            tried += R;
            __syncthreads();
        }
        if (lane < ns) {
            a.nid[i0 + lane] = t ? neg : c0;
            h.weight[i0 + lane] = t ? h.tw[t - 1] : 0.f;
            if (h.trials) h.trials[i0 + lane] = t;
            if (h.pos_score) h.pos_score[i0 + lane] = sp;
        }
        __syncthreads();
    }
}

int orx_launch_warpneg(orx_ctx* ctx, const WarpNegArgs& h) {
    if (h.s.n == 0) return ORX_OK;
    // experiments: samples per wavefront, slots per round, candidates per sample in the first round
    static const int s_env = getenv("ORX_WARP_CHUNK") ? atoi(getenv("ORX_WARP_CHUNK")) : 0;
    static const int b_env = getenv("ORX_WARP_SLOTS") ? atoi(getenv("ORX_WARP_SLOTS")) : 0;
    static const int r_env = getenv("ORX_WARP_FIRST") ? atoi(getenv("ORX_WARP_FIRST")) : 0;
    int S = s_env > 0 ? s_env : 16; if (S > 64) S = 64;
    int budget = b_env > 0 ? b_env : WN_SLOTS; if (budget > WN_SLOTS) budget = WN_SLOTS;
    int r0 = r_env > 0 ? r_env : 2; if (r0 > 256) r0 = 256;
    const int64_t nchunks = (h.s.n + S - 1) / S;
    int64_t g = nchunks; if (g > (int64_t)ctx->num_cu * 64) g = (int64_t)ctx->num_cu * 64;
    const dim3 grid((unsigned)g), block(64);
    const int D = h.D;
#define WN_LAUNCH(LPR, VEC)                                                                               \
    do {                                                                                                  \
        if (h.s.prop) ORX_LAUNCH(ctx, (warpneg_kernel<LPR, VEC, true>), grid, block, 0, h, S, budget, r0);    \
        else ORX_LAUNCH(ctx, (warpneg_kernel<LPR, VEC, false>), grid, block, 0, h, S, budget, r0);        \
    } while (0)
    if (D % 4 != 0 || D > 256) WN_LAUNCH(64, false);
    else if (D <= 4) WN_LAUNCH(1, true);
    else if (D <= 8) WN_LAUNCH(2, true);
    else if (D <= 16) WN_LAUNCH(4, true);
    else if (D <= 32) WN_LAUNCH(8, true);
    else if (D <= 64) WN_LAUNCH(16, true);
    else if (D <= 128) WN_LAUNCH(32, true);
    else WN_LAUNCH(64, true);
#undef WN_LAUNCH
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}
