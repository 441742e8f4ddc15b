// The fused pairwise step kernels (fused_kernel, fused_generic_kernel) and their launch dispatch, shared by two translation units:
// kernels_pairwise.hip instantiates them without per-triplet weights (every plain entry point), kernels_pairwise_weighted.hip with
// them (orx_pairwise_step_weighted) -- the two sets build side by side.  kernels_pairwise.hip's header comment has the design.
#pragma once
#include "orx_internal.h"

#include "orx_device.h"
#include "orx_apply_device.h"

// ------------------------------------------------------------ fused kernel ---
// LPR lanes own one row (D = 4*LPR).  MODE: see orx_internal.h.
// LONGGAP (lazy Adam): 0 = the merged replay loop, 1 = + the bounded per-row replay of rows far behind, 2 = the closed-form replay (orx_device.h AdamCF)
// WT: per-triplet weights (PairArgs::wt, orx_pairwise_step_weighted) -- a compile-time variant, so the kernels of the plain entry
// points are the code they were
// LOSS = false: the call asked for neither the loss nor the l2 sum (PairArgs::no_loss) -- g is computed as ever (the same score<>, its
// loss term unused), the l2 dot products, the two wavefront reductions and the store of the partial are gone.  Instantiated for the
// exact SGD step without weights only (launch_fused_mode); every other kernel computes its partials whether or not they are read
template <int LPR, int MODEL, int OPT, int MODE, bool CENSOR = false, bool STAGED = false, int LONGGAP = 0, bool WT = false, bool LOSS = true>
__global__ __launch_bounds__(256) void fused_kernel(PairArgs a) {
    constexpr int TPW = 64 / LPR;
    constexpr int D = 4 * LPR;
    // MODEL_BPR_NB: BPR with bp = bn = 0 as constants; no bias memory is touched (the bias pointers are NULL)
    constexpr bool NB = MODEL == MODEL_BPR_NB;
    constexpr int SM = NB ? (int)ORX_BPR : MODEL;      // the model of the score and the gradients
    // (SGD only.  Adagrad: 111 VGPRs with the pairing tail against 84 without -- a wavefront of occupancy; bounded to 96 registers
    // (`__launch_bounds__(256, 5)`: no spills) the kernel with pairs still takes 51.5 us against 49.6 without and the step 62.1
    // against 57.7, K = 20, one box: profiles/r5_adagrad_pairing_ab.txt -- the pair tail reads and writes the accumulator row too)
    constexpr bool PAIRS = MODE == MODE_EXACT && OPT == ORX_SGD && TPW > 1;
    __shared__ f4 pair_xg[PAIRS ? 256 : 1];            // pairing: gradient exchange, one slot per lane
    __shared__ float pair_xb[PAIRS && !NB ? 256 / LPR : 1];   // ... and per lane group (item bias)
    __shared__ f4 pair_xw[PAIRS ? 256 : 1];            // the writer's copy of the shared row as read
    __shared__ float pair_xwb[PAIRS && !NB ? 256 / LPR : 1];
    const int lane = threadIdx.x & 63;
    const int sub = lane % LPR;
    const int grp = lane / LPR;
    const int nab = MODE == MODE_EXACT ? a.n_apply_blocks : 0;
    if (MODE == MODE_EXACT && (int)blockIdx.x < nab) {          // apply role (block-uniform)
        inline_apply<LPR, OPT, CENSOR, STAGED, !NB>(a);
        return;
    }
    const int64_t wave_global = (int64_t)(blockIdx.x - nab) * 4 + (threadIdx.x >> 6);
    const int64_t stride = (int64_t)(gridDim.x - nab) * 4 * TPW;
    float loss_acc = 0.0f, sq_acc = 0.0f;

    for (int64_t t = wave_global * TPW + grp; t < a.B; t += stride) {
        // ids as rewritten by the plan: bit 31 = "row is referenced more than once", bits 30:29 = role of this reference among the row's
        // references (0 / 1 = plain store into scratch row 1 / 2, 2 = atomics or staging slot, 3 = no store: pairing), bit 28 = urgent.
        // The flags stay IN the id words and are tested where they are needed (six flag registers fewer per lane).
        uint32_t uw, pw, nw;
        // pairing (kernels_plan.hip): position t processes the triplet the plan put there -- one 16-byte record: its three ids, the
        // pairing word (this triplet shares a row with another lane group of this wavefront) and where the triplet stood (t0: its
        // staging records are indexed by that)
        uint32_t pi = 0u;
        int64_t t0 = t;
        bool packed = false;
        if (PAIRS) { packed = a.ids4 != nullptr; }
        if (packed) {
            const int4 v = a.ids4[t];
            uw = (uint32_t)v.x; pw = (uint32_t)v.y; nw = (uint32_t)v.z;
            pi = (uint32_t)v.w & 0x3ffu; t0 = (int64_t)((uint32_t)v.w >> 10);
        } else {
            uw = (uint32_t)a.uid[t]; pw = (uint32_t)a.pid[t]; nw = (uint32_t)a.nid[t];
        }
        const uint32_t idmask = MODE == MODE_EXACT ? (a.role_bits ? 0x0fffffffu : 0x7fffffffu) : 0xffffffffu;
        const int u = (int)(uw & idmask), p = (int)(pw & idmask), n = (int)(nw & idmask);
#define du FLAG_DUP(uw)
#define dp FLAG_DUP(pw)
#define dn FLAG_DUP(nw)
#define ku FLAG_ROLE(uw)
#define kp FLAG_ROLE(pw)
#define kn FLAG_ROLE(nw)
#define FLAG_DUP(w) (MODE == MODE_ACCUM ? 1 : (MODE == MODE_EXACT ? (int)((w) >> 31) : 0))
#define FLAG_ROLE(w) ((MODE == MODE_EXACT && a.role_bits) ? (int)(((w) >> 29) & 3u) : 2)
        // bitwise &: all three id loads are issued together (a short-circuit && lets the compiler
        // sink the loads behind each other: three dependent round trips)
        if (!(id_ok(u, a.NU) & id_ok(p, a.NI) & id_ok(n, a.NI))) {
            if (sub == 0) *a.err = 1;       // the reference's CPU gather raises; the triplet is skipped
            if (PAIRS) {
                if (pi & ORX_PAIR_VALID) {  // (its partner must not add what an earlier iteration left in LDS)
                    f4 z; z.x = z.y = z.z = z.w = 0.0f;
                    pair_xg[threadIdx.x] = z;
                    if (!NB && sub == 0) pair_xb[threadIdx.x / LPR] = 0.0f;
                }
            }
            continue;
        }
        // staged references (role 2 with a staging plan): slot = segment start of the row + rank of the
        // reference, looked up only where such a reference deposits its gradient
        const int64_t Bp = a.pid - a.uid;           // the three id arrays of a step are Bp apart
        auto slot_of = [&](int64_t ref) -> int {
            if (!STAGED) return -1;
            const int2 ri = a.refinfo[ref];
            return ri.x < 0 ? -1 : a.segstart[ri.x] + ri.y;      // (-1, 0): the row's range made no plan -> atomics
        };
        if (MODE == MODE_EXACT && nab && a.role_bits && (((uw | pw | nw) >> 28) & 1u)) {      // (the marks are made before the host knows whether the launch applies)
            // a row of this triplet is being updated by an apply block of this launch
            if (sub == 0) {
                if ((uw >> 28) & 1u) wait_ready(a.readyU + u, a.epoch);
                if ((pw >> 28) & 1u) wait_ready(a.readyV + p, a.epoch);
                if ((nw >> 28) & 1u) wait_ready(a.readyV + n, a.epoch);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        float* Up = a.U + (size_t)u * D + 4 * sub;
        float* Pp = a.V + (size_t)p * D + 4 * sub;
        float* Np = a.V + (size_t)n * D + 4 * sub;
        f4 ru = *reinterpret_cast<const f4*>(Up);
        f4 rp = *reinterpret_cast<const f4*>(Pp);
        f4 rn = *reinterpret_cast<const f4*>(Np);
        float bp = 0.f, bn = 0.f;
        if (!NB) { bp = a.b[p]; bn = a.b[n]; }
        // lazy Adam: (w, m, v) of the three rows and two biases, replayed up to the step before this one -- the
        // forward then sees exactly what the whole-table sweeps of TF 2.0 would have left
        f4 mu, vu, mp, vp, mn, vn;
        float mbp = 0.f, vbp = 0.f, mbn = 0.f, vbn = 0.f;
        if (OPT == ORX_ADAM) {
            const int T1 = a.step_t - 1;
            mu = *reinterpret_cast<const f4*>(a.aU + (size_t)u * D + 4 * sub); vu = *reinterpret_cast<const f4*>(a.a2U + (size_t)u * D + 4 * sub);
            mp = *reinterpret_cast<const f4*>(a.aV + (size_t)p * D + 4 * sub); vp = *reinterpret_cast<const f4*>(a.a2V + (size_t)p * D + 4 * sub);
            mn = *reinterpret_cast<const f4*>(a.aV + (size_t)n * D + 4 * sub); vn = *reinterpret_cast<const f4*>(a.a2V + (size_t)n * D + 4 * sub);
            if (!NB) { mbp = a.ab[p]; vbp = a.a2b[p]; mbn = a.ab[n]; vbn = a.a2b[n]; }
            // (the bias of an item shares the item row's stamp: the three tables are lazy together, api.hip)
            int lu = a.lastU[u], lp = a.lastV[p], ln = a.lastV[n];
            if (LONGGAP == 2) {
                const float4 Vt = a.lrv[T1];                 // (wave-uniform)
                AdamCF cf;
                if (lu < T1) { cf.setup(a.lrv, lu, T1, Vt, a.cf_lb1, a.cf_lb2); cf.row4(ru, mu, vu, a.eps, a.cf_delta); }
                if (lp < T1) { cf.setup(a.lrv, lp, T1, Vt, a.cf_lb1, a.cf_lb2); cf.row4(rp, mp, vp, a.eps, a.cf_delta); if (!NB) cf.elem(bp, mbp, vbp, a.eps, a.cf_delta); }
                if (ln < T1) { cf.setup(a.lrv, ln, T1, Vt, a.cf_lb1, a.cf_lb2); cf.row4(rn, mn, vn, a.eps, a.cf_delta); if (!NB) cf.elem(bn, mbn, vbn, a.eps, a.cf_delta); }
                lu = lp = ln = T1;
            }
            if (LONGGAP == 1) {      // large tables: rows that have waited very long take the bounded replay and leave the merged loop
                if (T1 - lu > ORX_ADAM_LONG_GAP) {
                    float z0 = 0.f, z1 = 0.f, z2 = 0.f;
                    adam_replay4_bounded(ru, mu, vu, z0, z1, z2, lu, T1, a.lrt, a.b1, a.b2, a.eps);
                    lu = T1;
                }
                if (T1 - lp > ORX_ADAM_LONG_GAP) { adam_replay4_bounded(rp, mp, vp, bp, mbp, vbp, lp, T1, a.lrt, a.b1, a.b2, a.eps); lp = T1; }
                if (T1 - ln > ORX_ADAM_LONG_GAP) { adam_replay4_bounded(rn, mn, vn, bn, mbn, vbn, ln, T1, a.lrt, a.b1, a.b2, a.eps); ln = T1; }
            }
            if (LONGGAP == 2) {}
            else if (a.newton) adam_catchup_triplet<true, LPR>(ru, mu, vu, lu, rp, mp, vp, lp, rn, mn, vn, ln, bp, mbp, vbp, bn, mbn, vbn, T1, a.lrt, a.b1, a.b2, a.eps);
            else adam_catchup_triplet<false, LPR>(ru, mu, vu, lu, rp, mp, vp, lp, rn, mn, vn, ln, bp, mbp, vbp, bn, mbn, vbn, T1, a.lrt, a.b1, a.b2, a.eps);
        }

        const float red = group_allreduce<LPR>(score_partial<SM>(ru, rp, rn));
        float term, g;
        // per-triplet weight (orx_pairwise_step_weighted, score_weighted): it scales the loss term and g together; read at the triplet's ORIGINAL position --
        // the caller's array knows nothing of the plan's reordering.  !WT: the plain 1/B of every other entry point
        if (WT) score_weighted<SM>(red, NB ? 0.f : bp, NB ? 0.f : bn, a.invB, a.wt[t0], a.margin, term, g);
        else score<SM>(red, NB ? 0.f : bp, NB ? 0.f : bn, a.invB, a.margin, term, g);
        if (LOSS) {
            sq_acc += dot4(ru, ru) + dot4(rp, rp) + dot4(rn, rn);
            if (sub == 0) loss_acc += term;
        }
        if (MODE == MODE_LOSS) continue;

        f4 gu, gp, gn; float gbp, gbn;
        row_grads<SM>(ru, rp, rn, g, a.l2w, gu, gp, gn, gbp, gbn);

        // pairing: the two lane groups that share a row leave their gradient of it in LDS (one slot per lane; a wavefront's LDS
        // operations execute in order, so no barrier), the WRITER also the row and bias it read; for both the slot is then settled
        // (role 3: no store below).  After the other stores (pair_tail) the writer sums the two gradients -- TF sums the gradients
        // of duplicate indices before the sparse apply -- and updates the row as the unique row it has become.
        if (PAIRS) {
            if (pi & ORX_PAIR_VALID) {
                const int myslot = (pi >> 4) & 3;
                pair_xg[threadIdx.x] = myslot == 0 ? gu : (myslot == 1 ? gp : gn);
                if (pi & ORX_PAIR_WRITER) pair_xw[threadIdx.x] = myslot == 0 ? ru : (myslot == 1 ? rp : rn);
                if (!NB && sub == 0) {
                    pair_xb[threadIdx.x / LPR] = myslot == 1 ? gbp : gbn;
                    if (pi & ORX_PAIR_WRITER) pair_xwb[threadIdx.x / LPR] = myslot == 1 ? bp : bn;
                }
                if (myslot == 0) uw |= 0xe0000000u;         // duplicate flag + role 3
                else if (myslot == 1) pw |= 0xe0000000u;
                else nw |= 0xe0000000u;
            }
        }
        auto pair_tail = [&]() {
            if (!PAIRS) return;
            if (!(pi & ORX_PAIR_WRITER)) return;
            const int myslot = (pi >> 4) & 3, oslot = (pi >> 6) & 3;
            const int xsrc = (int)(threadIdx.x & ~63u) + (int)(pi & 15u) * LPR + sub;
            const int id = reinterpret_cast<const int*>(a.ids4 + t)[myslot] & 0x0fffffff;      // (the tail keeps nothing of the triplet alive but t and its pairing word)
            const size_t off = (size_t)id * D + 4 * sub;
            float* W = myslot == 0 ? a.U : a.V;
            float* A = myslot == 0 ? a.aU : a.aV;
            const f4 gs = pair_xg[threadIdx.x] + pair_xg[xsrc];
            const f4 w = pair_xw[threadIdx.x];
            if (CENSOR) {
                f4 wn = censor4<LPR>(opt_new4<OPT>(A + off, w, gs, a.lr, a.eps), a.min_norm);
                // a positive of one triplet and a negative of the other: censored once per id list (ucml.py:46-48)
                if (myslot != oslot) wn = censor4<LPR>(wn, a.min_norm);
                *reinterpret_cast<f4*>(W + off) = wn;
            } else {
                opt_apply4<OPT>(W + off, A + off, w, gs, a.lr, a.eps);
            }
            if (!NB && myslot != 0 && sub == 0)
                opt_apply1<OPT>(a.b + id, a.ab + id, pair_xwb[threadIdx.x / LPR], pair_xb[threadIdx.x / LPR] + pair_xb[xsrc / LPR], a.lr, a.eps);
        };

        if (OPT == ORX_ADAM) {
            // a row referenced once takes its step here (replayed state + gradient), a duplicated one deposits the gradient
            const float lrT = a.lrt[a.step_t];
            if (du == 0) {
                adam_elem4(ru, mu, vu, gu, lrT, a.b1, a.b2, a.eps);
                if (CENSOR) ru = censor4<LPR>(ru, a.min_norm);      // censor_vec fused into the write-back (see below)
                *reinterpret_cast<f4*>(Up) = ru; *reinterpret_cast<f4*>(a.aU + (size_t)u * D + 4 * sub) = mu;
                *reinterpret_cast<f4*>(a.a2U + (size_t)u * D + 4 * sub) = vu;
                if (sub == 0) a.lastU[u] = a.step_t;
            } else dup_store4s(a.gU, a.gU2, (size_t)u * D + 4 * sub, gu, ku, a.stage, ku == 2 ? slot_of(t0) : -1, D, sub);
            if (dp == 0) {
                adam_elem4(rp, mp, vp, gp, lrT, a.b1, a.b2, a.eps);
                if (CENSOR) rp = censor4<LPR>(rp, a.min_norm);
                *reinterpret_cast<f4*>(Pp) = rp; *reinterpret_cast<f4*>(a.aV + (size_t)p * D + 4 * sub) = mp;
                *reinterpret_cast<f4*>(a.a2V + (size_t)p * D + 4 * sub) = vp;
                if (sub == 0) {
                    if (!NB) { adam_elem(bp, mbp, vbp, gbp, lrT, a.b1, a.b2, a.eps); a.b[p] = bp; a.ab[p] = mbp; a.a2b[p] = vbp; }
                    a.lastV[p] = a.step_t;
                    if (!NB) a.lastb[p] = a.step_t;
                }
            } else {
                const int sp = kp == 2 ? slot_of(Bp + t0) : -1;
                dup_store4s(a.gV, a.gV2, (size_t)p * D + 4 * sub, gp, kp, a.stage, sp, D, sub);
                if (sub == 0) { if (!NB) dup_store1s(a.gb, a.gb2, p, gbp, kp, a.stageb, sp); if (CENSOR) a.sideV[2 * (size_t)p] = a.epoch; }
            }
            if (dn == 0) {
                adam_elem4(rn, mn, vn, gn, lrT, a.b1, a.b2, a.eps);
                if (CENSOR) rn = censor4<LPR>(rn, a.min_norm);
                *reinterpret_cast<f4*>(Np) = rn; *reinterpret_cast<f4*>(a.aV + (size_t)n * D + 4 * sub) = mn;
                *reinterpret_cast<f4*>(a.a2V + (size_t)n * D + 4 * sub) = vn;
                if (sub == 0) {
                    if (!NB) { adam_elem(bn, mbn, vbn, gbn, lrT, a.b1, a.b2, a.eps); a.b[n] = bn; a.ab[n] = mbn; a.a2b[n] = vbn; }
                    a.lastV[n] = a.step_t;
                    if (!NB) a.lastb[n] = a.step_t;
                }
            } else {
                const int sn = kn == 2 ? slot_of(2 * Bp + t0) : -1;
                dup_store4s(a.gV, a.gV2, (size_t)n * D + 4 * sub, gn, kn, a.stage, sn, D, sub);
                if (sub == 0) { if (!NB) dup_store1s(a.gb, a.gb2, n, gbn, kn, a.stageb, sn); if (CENSOR) a.sideV[2 * (size_t)n + 1] = a.epoch; }
            }
            continue;
        }
        // unique row: in place.  duplicated row: gradient into gsum, row untouched.
        if (CENSOR) {
            // censor_vec fused into the write-back: a row referenced once is censored once, here;
            // duplicated rows are censored by the kernel that applies their summed gradient
            f4 wu = ru, wp = rp, wn = rn;
            if (du == 0) wu = opt_new4<OPT>(a.aU + (size_t)u * D + 4 * sub, ru, gu, a.lr, a.eps);
            else dup_store4s(a.gU, a.gU2, (size_t)u * D + 4 * sub, gu, ku, a.stage, ku == 2 ? slot_of(t0) : -1, D, sub);
            if (dp == 0) {
                wp = opt_new4<OPT>(a.aV + (size_t)p * D + 4 * sub, rp, gp, a.lr, a.eps);
                if (sub == 0) opt_apply1<OPT>(a.b + p, a.ab + p, bp, gbp, a.lr, a.eps);
            } else {
                const int sp = kp == 2 ? slot_of(Bp + t0) : -1;
                dup_store4s(a.gV, a.gV2, (size_t)p * D + 4 * sub, gp, kp, a.stage, sp, D, sub);
                if (sub == 0) { dup_store1s(a.gb, a.gb2, p, gbp, kp, a.stageb, sp); if (kp != 3) a.sideV[2 * (size_t)p] = a.epoch; }
            }
            if (dn == 0) {
                wn = opt_new4<OPT>(a.aV + (size_t)n * D + 4 * sub, rn, gn, a.lr, a.eps);
                if (sub == 0) opt_apply1<OPT>(a.b + n, a.ab + n, bn, gbn, a.lr, a.eps);
            } else {
                const int sn = kn == 2 ? slot_of(2 * Bp + t0) : -1;
                dup_store4s(a.gV, a.gV2, (size_t)n * D + 4 * sub, gn, kn, a.stage, sn, D, sub);
                if (sub == 0) { dup_store1s(a.gb, a.gb2, n, gbn, kn, a.stageb, sn); if (kn != 3) a.sideV[2 * (size_t)n + 1] = a.epoch; }
            }
            wu = censor4<LPR>(wu, a.min_norm); wp = censor4<LPR>(wp, a.min_norm); wn = censor4<LPR>(wn, a.min_norm);
            if (du == 0) *reinterpret_cast<f4*>(Up) = wu;
            if (dp == 0) *reinterpret_cast<f4*>(Pp) = wp;
            if (dn == 0) *reinterpret_cast<f4*>(Np) = wn;
            pair_tail();
            continue;
        }
        if (du == 0) opt_apply4<OPT>(Up, a.aU + (size_t)u * D + 4 * sub, ru, gu, a.lr, a.eps);
        else dup_store4s(a.gU, a.gU2, (size_t)u * D + 4 * sub, gu, ku, a.stage, ku == 2 ? slot_of(t0) : -1, D, sub);
        if (dp == 0) {
            opt_apply4<OPT>(Pp, a.aV + (size_t)p * D + 4 * sub, rp, gp, a.lr, a.eps);
            if (!NB && sub == 0) opt_apply1<OPT>(a.b + p, a.ab + p, bp, gbp, a.lr, a.eps);
        } else {
            const int sp = kp == 2 ? slot_of(Bp + t0) : -1;
            dup_store4s(a.gV, a.gV2, (size_t)p * D + 4 * sub, gp, kp, a.stage, sp, D, sub);
            if (!NB && sub == 0) dup_store1s(a.gb, a.gb2, p, gbp, kp, a.stageb, sp);
        }
        if (dn == 0) {
            opt_apply4<OPT>(Np, a.aV + (size_t)n * D + 4 * sub, rn, gn, a.lr, a.eps);
            if (!NB && sub == 0) opt_apply1<OPT>(a.b + n, a.ab + n, bn, gbn, a.lr, a.eps);
        } else {
            const int sn = kn == 2 ? slot_of(2 * Bp + t0) : -1;
            dup_store4s(a.gV, a.gV2, (size_t)n * D + 4 * sub, gn, kn, a.stage, sn, D, sub);
            if (!NB && sub == 0) dup_store1s(a.gb, a.gb2, n, gbn, kn, a.stageb, sn);
        }
        pair_tail();
    }
#undef du
#undef dp
#undef dn
#undef ku
#undef kp
#undef kn
#undef FLAG_DUP
#undef FLAG_ROLE
    if (!LOSS) return;
    const float ls = wave_sum(loss_acc);
    const float sq = wave_sum(sq_acc);
    if (lane == 0) {
        float2 v; v.x = ls; v.y = 0.5f * sq;
        *reinterpret_cast<float2*>(a.partial + 2 * wave_global) = v;
    }
}

// Any D: one triplet per wavefront, scalar elements strided by 64 lanes, two
// passes over the (L1/L2-resident) rows.  Used for dims without a float4 path
// (e.g. the example's dim_embed = 50, tf2_examples/bpr_citeulike.py:12).
template <int MODEL, int OPT, int MODE, bool WT = false>
__global__ __launch_bounds__(256) void fused_generic_kernel(PairArgs a) {
    constexpr bool NB = MODEL == MODEL_BPR_NB;         // BPR without item biases (see fused_kernel)
    constexpr int SM = NB ? (int)ORX_BPR : MODEL;
    const int lane = threadIdx.x & 63;
    const int D = a.D;
    const int64_t wave_global = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t stride = (int64_t)gridDim.x * 4;
    float loss_acc = 0.0f, sq_acc = 0.0f;
    for (int64_t t = wave_global; t < a.B; t += stride) {
        int u = a.uid[t], p = a.pid[t], n = a.nid[t];
        int du = 0, dp = 0, dn = 0;
        int ku = 2, kp = 2, kn = 2;     // duplicate role: 0 / 1 = plain store into scratch row 1 / 2, 2 = atomics
        if (MODE == MODE_EXACT) {       // ids rewritten by dedup_kernel: bit 31 = "row is referenced more than once"
            du = (uint32_t)u >> 31; dp = (uint32_t)p >> 31; dn = (uint32_t)n >> 31;
            if (a.role_bits) {          // bits 30:29 = role of this reference among the row's references
                ku = ((uint32_t)u >> 29) & 3; kp = ((uint32_t)p >> 29) & 3; kn = ((uint32_t)n >> 29) & 3;
                u &= 0x1fffffff; p &= 0x1fffffff; n &= 0x1fffffff;
            } else {
                u &= 0x7fffffff; p &= 0x7fffffff; n &= 0x7fffffff;
            }
        }
        if (MODE == MODE_ACCUM) { du = dp = dn = 1; }
        // bitwise &: all three id loads are issued together (a short-circuit && lets the compiler
        // sink the loads behind each other: three dependent round trips)
        if (!(id_ok(u, a.NU) & id_ok(p, a.NI) & id_ok(n, a.NI))) {
            if (lane == 0) *a.err = 1;
            continue;
        }
        float* Ur = a.U + (size_t)u * D;
        float* Pr = a.V + (size_t)p * D;
        float* Nr = a.V + (size_t)n * D;
        const float bp = NB ? 0.f : a.b[p], bn = NB ? 0.f : a.b[n];
        float part = 0.0f;
        for (int e = lane; e < D; e += 64) {
            const float x = Ur[e], y = Pr[e], z = Nr[e];
            if (SM == ORX_BPR) part += x * (y - z);
            else part += (x - z) * (x - z) - (x - y) * (x - y);
            sq_acc += x * x + y * y + z * z;
        }
        const float red = wave_sum(part);
        float term, g;
        if (WT) score_weighted<SM>(red, bp, bn, a.invB, a.wt[t], a.margin, term, g);      // (per-triplet weight, see fused_kernel; no pairing on this path)
        else score<SM>(red, bp, bn, a.invB, a.margin, term, g);
        if (lane == 0) loss_acc += term;
        if (MODE == MODE_LOSS) continue;
        for (int e = lane; e < D; e += 64) {
            const float x = Ur[e], y = Pr[e], z = Nr[e];
            float gu, gp, gn;
            if (SM == ORX_BPR) {
                gu = g * (y - z) + a.l2w * x; gp = g * x + a.l2w * y; gn = -g * x + a.l2w * z;
            } else {
                const float a2 = 2.0f * g;
                gu = -a2 * (y - z) + a.l2w * x; gp = -a2 * (x - y) + a.l2w * y; gn = a2 * (x - z) + a.l2w * z;
            }
            if (du == 0) opt_apply1<OPT>(Ur + e, a.aU + (size_t)u * D + e, x, gu, a.lr, a.eps);
            else dup_store1(a.gU, a.gU2, (size_t)u * D + e, gu, ku);
            if (dp == 0) opt_apply1<OPT>(Pr + e, a.aV + (size_t)p * D + e, y, gp, a.lr, a.eps);
            else dup_store1(a.gV, a.gV2, (size_t)p * D + e, gp, kp);
            if (dn == 0) opt_apply1<OPT>(Nr + e, a.aV + (size_t)n * D + e, z, gn, a.lr, a.eps);
            else dup_store1(a.gV, a.gV2, (size_t)n * D + e, gn, kn);
        }
        const float gbp = SM == ORX_BPR ? g : -g, gbn = -gbp;
        if (!NB && lane == 0) {
            if (dp == 0) opt_apply1<OPT>(a.b + p, a.ab + p, bp, gbp, a.lr, a.eps);
            else dup_store1(a.gb, a.gb2, p, gbp, kp);
            if (dn == 0) opt_apply1<OPT>(a.b + n, a.ab + n, bn, gbn, a.lr, a.eps);
            else dup_store1(a.gb, a.gb2, n, gbn, kn);
        }
    }
    const float ls = wave_sum(loss_acc);
    const float sq = wave_sum(sq_acc);
    if (lane == 0) {
        float2 v; v.x = ls; v.y = 0.5f * sq;
        *reinterpret_cast<float2*>(a.partial + 2 * wave_global) = v;
    }
}

// ---------------------------------------------------------------- launchers ---
static inline int lpr_for_dim(int D) {
    switch (D) {
        case 16: return 4;
        case 32: return 8;
        case 64: return 16;
        case 128: return 32;
        case 256: return 64;
        default: return 0;      // generic path
    }
}

static inline int64_t fused_grid(int D, int64_t B) {
    const int lpr = lpr_for_dim(D);
    const int64_t tpb = lpr ? 4 * (64 / lpr) : 4;      // triplets per 256-thread block per pass
    int64_t g = (B + tpb - 1) / tpb;
    const int64_t cap = 1 << 16;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return g;
}

template <bool WT, int LPR, int MODEL, int OPT>
static void launch_fused_mode(int mode, dim3 g, orx_ctx* s, const PairArgs& a) {
    constexpr bool CEN = MODEL != MODEL_BPR_NB;      // censor instantiations (UCML's censor_vec; bias-free BPR has none)
    switch (mode) {
        case MODE_EXACT:
            if constexpr (!WT && OPT == ORX_SGD) {      // the loss-free forms (fused_kernel LOSS = false): the headline and the UCML + censor workload take them
                if (a.no_loss) {
                    if (CEN && a.censor && a.stage) ORX_LAUNCH(s, (fused_kernel<LPR, MODEL, OPT, MODE_EXACT, CEN, true, 0, false, false>), g, dim3(256), 0, a);
                    else if (CEN && a.censor) ORX_LAUNCH(s, (fused_kernel<LPR, MODEL, OPT, MODE_EXACT, CEN, false, 0, false, false>), g, dim3(256), 0, a);
                    else if (a.stage) ORX_LAUNCH(s, (fused_kernel<LPR, MODEL, OPT, MODE_EXACT, false, true, 0, false, false>), g, dim3(256), 0, a);
                    else ORX_LAUNCH(s, (fused_kernel<LPR, MODEL, OPT, MODE_EXACT, false, false, 0, false, false>), g, dim3(256), 0, a);
                    break;
                }
            }
            if (CEN && a.censor && a.stage) ORX_LAUNCH(s, (fused_kernel<LPR, MODEL, OPT, MODE_EXACT, CEN, true, 0, WT>), g, dim3(256), 0, a);
            else if (CEN && a.censor) ORX_LAUNCH(s, (fused_kernel<LPR, MODEL, OPT, MODE_EXACT, CEN, false, 0, WT>), g, dim3(256), 0, a);
            else if (a.stage) ORX_LAUNCH(s, (fused_kernel<LPR, MODEL, OPT, MODE_EXACT, false, true, 0, WT>), g, dim3(256), 0, a);
            else ORX_LAUNCH(s, (fused_kernel<LPR, MODEL, OPT, MODE_EXACT, false, false, 0, WT>), g, dim3(256), 0, a);
            break;
        case MODE_HOGWILD: if constexpr (!WT) ORX_LAUNCH(s, (fused_kernel<LPR, MODEL, OPT, MODE_HOGWILD, false, false, 0, false>), g, dim3(256), 0, a); break;      // (the weighted step refuses hogwild)
        case MODE_ACCUM: ORX_LAUNCH(s, (fused_kernel<LPR, MODEL, ORX_SGD, MODE_ACCUM, false, false, 0, WT>), g, dim3(256), 0, a); break;
        default: ORX_LAUNCH(s, (fused_kernel<LPR, MODEL, ORX_SGD, MODE_LOSS, false, false, 0, WT>), g, dim3(256), 0, a); break;
    }
}

template <bool WT, int MODEL, int OPT>
static void launch_generic_mode(int mode, dim3 g, orx_ctx* s, const PairArgs& a) {
    switch (mode) {
        case MODE_EXACT: ORX_LAUNCH(s, (fused_generic_kernel<MODEL, OPT, MODE_EXACT, WT>), g, dim3(256), 0, a); break;
        case MODE_HOGWILD: if constexpr (!WT) ORX_LAUNCH(s, (fused_generic_kernel<MODEL, OPT, MODE_HOGWILD, false>), g, dim3(256), 0, a); break;
        case MODE_ACCUM: ORX_LAUNCH(s, (fused_generic_kernel<MODEL, ORX_SGD, MODE_ACCUM, WT>), g, dim3(256), 0, a); break;
        default: ORX_LAUNCH(s, (fused_generic_kernel<MODEL, ORX_SGD, MODE_LOSS, WT>), g, dim3(256), 0, a); break;
    }
}

template <bool WT, int MODEL, int OPT>
static void launch_fused_lpr(int lpr, int mode, dim3 g, orx_ctx* s, const PairArgs& a) {
    switch (lpr) {
        case 4: launch_fused_mode<WT, 4, MODEL, OPT>(mode, g, s, a); break;
        case 8: launch_fused_mode<WT, 8, MODEL, OPT>(mode, g, s, a); break;
        case 16: launch_fused_mode<WT, 16, MODEL, OPT>(mode, g, s, a); break;
        case 32: launch_fused_mode<WT, 32, MODEL, OPT>(mode, g, s, a); break;
        case 64: launch_fused_mode<WT, 64, MODEL, OPT>(mode, g, s, a); break;
        default: launch_generic_mode<WT, MODEL, OPT>(mode, g, s, a); break;
    }
}

// lazy Adam (exact mode, float4 dims): its own small set of instantiations
template <bool WT, int MODEL>
static void launch_fused_adam(int lpr, dim3 g, orx_ctx* s, const PairArgs& a) {
#define ORX_FC(L) do { if (a.stage) ORX_LAUNCH(s, (fused_kernel<L, MODEL, ORX_ADAM, MODE_EXACT, false, true, 2, WT>), g, dim3(256), 0, a); \
                       else ORX_LAUNCH(s, (fused_kernel<L, MODEL, ORX_ADAM, MODE_EXACT, false, false, 2, WT>), g, dim3(256), 0, a); } while (0)
    if (a.lrv != nullptr && !a.censor) {      // the closed-form replay (orx_device.h AdamCF): no loop over the skipped steps
        switch (lpr) {
            case 4: ORX_FC(4); break;
            case 8: ORX_FC(8); break;
            case 16: ORX_FC(16); break;
            case 32: ORX_FC(32); break;
            default: ORX_FC(64); break;
        }
        return;
    }
#undef ORX_FC
#define ORX_FL(L) do { if (a.stage) ORX_LAUNCH(s, (fused_kernel<L, MODEL, ORX_ADAM, MODE_EXACT, false, true, 1, WT>), g, dim3(256), 0, a); \
                       else ORX_LAUNCH(s, (fused_kernel<L, MODEL, ORX_ADAM, MODE_EXACT, false, false, 1, WT>), g, dim3(256), 0, a); } while (0)
    if (a.long_gap && !a.censor) {      // tables large relative to the batch: the variant with the bounded per-row replay
        switch (lpr) {
            case 4: ORX_FL(4); break;
            case 8: ORX_FL(8); break;
            case 16: ORX_FL(16); break;
            case 32: ORX_FL(32); break;
            default: ORX_FL(64); break;
        }
        return;
    }
#undef ORX_FL
    constexpr bool CEN = MODEL != MODEL_BPR_NB;      // (see launch_fused_mode)
#define ORX_FA(L) do { if (CEN && a.censor) { if (a.stage) ORX_LAUNCH(s, (fused_kernel<L, MODEL, ORX_ADAM, MODE_EXACT, CEN, true, 0, WT>), g, dim3(256), 0, a); \
                                         else ORX_LAUNCH(s, (fused_kernel<L, MODEL, ORX_ADAM, MODE_EXACT, CEN, false, 0, WT>), g, dim3(256), 0, a); } \
                       else if (a.stage) ORX_LAUNCH(s, (fused_kernel<L, MODEL, ORX_ADAM, MODE_EXACT, false, true, 0, WT>), g, dim3(256), 0, a); \
                       else ORX_LAUNCH(s, (fused_kernel<L, MODEL, ORX_ADAM, MODE_EXACT, false, false, 0, WT>), g, dim3(256), 0, a); } while (0)
    switch (lpr) {
        case 4: ORX_FA(4); break;
        case 8: ORX_FA(8); break;
        case 16: ORX_FA(16); break;
        case 32: ORX_FA(32); break;
        default: ORX_FA(64); break;
    }
#undef ORX_FA
}

// the launch of one fused step, with (WT) or without per-triplet weights: orx_launch_fused / orx_launch_fused_weighted
template <bool WT>
static int launch_fused_any(orx_ctx* ctx, int model, int optkind, int mode, const PairArgs& a) {
    ProfScope ps(ctx, ORX_K_FUSED);
    const int lpr = lpr_for_dim(a.D);
    const dim3 g((unsigned)(fused_grid(a.D, a.B) + (mode == MODE_EXACT ? a.n_apply_blocks : 0)));
    if (optkind == ORX_ADAM && mode == MODE_EXACT) {
        ORX_ARG(lpr != 0 && a.lrt != nullptr, "fused: the lazy Adam path needs a float4 dim");
        if (model == ORX_BPR) launch_fused_adam<WT, ORX_BPR>(lpr, g, ctx, a);
        else if (model == MODEL_BPR_NB) launch_fused_adam<WT, MODEL_BPR_NB>(lpr, g, ctx, a);
        else launch_fused_adam<WT, ORX_UCML>(lpr, g, ctx, a);
        ORX_HIP(hipGetLastError());
        return ORX_OK;
    }
    const int ok = (optkind == ORX_ADAGRAD || optkind == ORX_MOMENTUM) ? optkind : ORX_SGD;
    // momentum: exact mode only (the host refuses hogwild), the rest of its mode switch is never taken
    if (ok == ORX_MOMENTUM && mode != MODE_EXACT) {
        orx_set_error("fused: momentum takes the exact mode only (mode %d)", mode);
        return ORX_ERR_ARG;
    }
    if (model == ORX_BPR) {
        if (ok == ORX_ADAGRAD) launch_fused_lpr<WT, ORX_BPR, ORX_ADAGRAD>(lpr, mode, g, ctx, a);
        else if (ok == ORX_MOMENTUM) launch_fused_lpr<WT, ORX_BPR, ORX_MOMENTUM>(lpr, mode, g, ctx, a);
        else launch_fused_lpr<WT, ORX_BPR, ORX_SGD>(lpr, mode, g, ctx, a);
    } else if (model == MODEL_BPR_NB) {
        if (ok == ORX_ADAGRAD) launch_fused_lpr<WT, MODEL_BPR_NB, ORX_ADAGRAD>(lpr, mode, g, ctx, a);
        else if (ok == ORX_MOMENTUM) launch_fused_lpr<WT, MODEL_BPR_NB, ORX_MOMENTUM>(lpr, mode, g, ctx, a);
        else launch_fused_lpr<WT, MODEL_BPR_NB, ORX_SGD>(lpr, mode, g, ctx, a);
    } else {
        if (ok == ORX_ADAGRAD) launch_fused_lpr<WT, ORX_UCML, ORX_ADAGRAD>(lpr, mode, g, ctx, a);
        else if (ok == ORX_MOMENTUM) launch_fused_lpr<WT, ORX_UCML, ORX_MOMENTUM>(lpr, mode, g, ctx, a);
        else launch_fused_lpr<WT, ORX_UCML, ORX_SGD>(lpr, mode, g, ctx, a);
    }
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}
