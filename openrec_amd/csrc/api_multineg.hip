// C-ABI entry points of the one-positive-against-N-negatives objective: orx_multineg_step and orx_multineg_loss
// (include/openrec_hip.h has the semantics, kernels_multineg.hip the kernels; orx_sampler_pairwise_multi, which delivers the
// negatives, is in api_sampler.hip).
//
// Per step: the touch of (uid; pid, nid), ONE gradient launch that writes per-occurrence gradient rows and the concatenated item id
// list pid | nid, [Adam: the counter advances], then orx_apply_rows of the user table and of the item table with the bias.  The
// gradient launch ends before the applies begin, so every gradient is taken on the pre-step tables.  nid and neg_offset are lists
// of width N.  (The loss sums are loss_reduce's, not orx_launch_loss_accumulate's: that one adds its blocks' sums with fp64
// atomics once there are more than 2048 partials, which would cost loss_out its bit-repeatability.)
#include <cstring>

#include "orx_internal.h"

// what the step and the forward check beyond the shared checks
static int check_kind(const char* fn, int kind, int32_t N) {
    ORX_ARG(kind == ORX_MN_SOFTMAX || kind == ORX_MN_LOGSIG, "%s: unknown loss kind %d (ORX_MN_SOFTMAX, ORX_MN_LOGSIG)", fn, kind);
    ORX_ARG(N >= 1 && N <= 64, "%s: N must be in [1, 64], got %d", fn, N);
    return ORX_OK;
}

// the step-independent part of the kernel's arguments
static MultiNegArgs model_args(orx_ctx* c, orx_table* U, orx_table* V, orx_table* b, int64_t B, int32_t N, float l2w) {
    MultiNegArgs a;
    memset(&a, 0, sizeof(a));
    a.U = U->w; a.V = V->w; a.b = b ? b->w : nullptr;
    a.B = B; a.NU = U->rows; a.NI = V->rows; a.N = N; a.D = U->dim; a.gs = (U->dim + 1 + 3) & ~3;
    a.invB = 1.0f / (float)B; a.l2w = l2w; a.err = c->d_err;
    return a;
}

extern "C" int orx_multineg_step(orx_ctx* c, int kind, orx_opt* opt, orx_table* U, orx_table* V, orx_table* b,
                                 const int32_t* uid, const int32_t* pid, const int32_t* nid, const float* weight, const float* neg_offset,
                                 int64_t K, int64_t B, int32_t N, int64_t id_stride, float l2_reg, int flags,
                                 float* loss_out, float* l2_out) {
    static const char* fn = "orx_multineg_step";
    CHECK(orx_check_dot_step(fn, c, opt, U, V, b, 0, K, B, id_stride, l2_reg, flags, ~0));
    CHECK(check_kind(fn, kind, N));
    if (K == 0 || B == 0) return ORX_OK;
    ORX_ARG(uid && pid && nid, "%s: NULL id pointer", fn);
    ORX_ARG((B * (1 + (int64_t)N)) <= 0x7fffffffLL, "%s: B * (1 + N) must fit 31 bits", fn);
    ORX_HIP(hipSetDevice(c->device));

    StepInputs in;
    CHECK(orx_stage_steps(c, K, B, id_stride, flags, {{uid, 1}, {pid, 1}, {nid, N}}, {{weight, 1}, {neg_offset, N}}, &in));
    MultiNegArgs a = model_args(c, U, V, b, B, N, l2_reg);
    const int gs = a.gs;
    const int64_t nI = B * (1 + (int64_t)N);
    // scratch, one buffer reused by every step: the concatenated item ids, the gradient rows
    Carve cv;
    const size_t o_list = cv.take((size_t)nI * sizeof(int32_t));
    const size_t o_gu = cv.take((size_t)B * gs * sizeof(float));
    const size_t o_gi = cv.take((size_t)nI * gs * sizeof(float));
    ENSURE(c->d_tmp, c->d_tmp_cap, cv.off);
    char* base = reinterpret_cast<char*>(c->d_tmp);
    a.list = reinterpret_cast<int32_t*>(base + o_list);
    a.gu = reinterpret_cast<float*>(base + o_gu); a.gi = reinterpret_cast<float*>(base + o_gi);
    orx_table* tabs[3] = {U, V, b};
    const int ntabs = b ? 3 : 2;

    return orx_run_steps(c, K, orx_multineg_nwaves(c, a.D, B), flags, loss_out, l2_out, nullptr, [&](int64_t s, int64_t, float* partial) -> int {
        a.uid = in.id[0] + s * in.ds; a.pid = in.id[1] + s * in.ds; a.nid = in.id[2] + s * in.ds * N;
        a.wt = in.f[0] ? in.f[0] + s * in.ds : nullptr;
        a.off = in.f[1] ? in.f[1] + s * in.ds * N : nullptr;
        a.partial = partial;
        CHECK(orx_touch_step(U, V, b, a.uid, B, a.pid, B, a.nid, B * N));
        CHECK(orx_launch_multineg(c, kind, true, a));
        if (opt->kind == ORX_ADAM) CHECK(orx_opt_advance(opt, tabs, ntabs));      // once per step: after the step's reads, before its applies
        CHECK(orx_apply_rows(c, opt, U, nullptr, a.uid, B, a.gu, gs));
        return orx_apply_rows(c, opt, V, b, a.list, nI, a.gi, gs);
    });
}

extern "C" int orx_multineg_loss(orx_ctx* c, int kind, orx_table* U, orx_table* V, orx_table* b,
                                 const int32_t* uid, const int32_t* pid, const int32_t* nid, const float* weight, const float* neg_offset,
                                 int64_t B, int32_t N, int flags, float* loss_out, float* l2_out) {
    static const char* fn = "orx_multineg_loss";
    CHECK(orx_check_dot_model(fn, c, U, V, b, 0, 0, 0));
    CHECK(check_kind(fn, kind, N));
    ORX_ARG((flags & ~ORX_IDS_DEVICE) == 0, "%s: flags other than ORX_IDS_DEVICE", fn);
    ORX_ARG(B >= 0, "%s: negative B", fn);
    if (B == 0) {
        if (loss_out) *loss_out = 0.f;
        if (l2_out) *l2_out = 0.f;
        return ORX_OK;
    }
    ORX_ARG(uid && pid && nid, "%s: NULL id pointer", fn);
    ORX_HIP(hipSetDevice(c->device));
    StepInputs in;
    CHECK(orx_stage_steps(c, 1, B, B, flags, {{uid, 1}, {pid, 1}, {nid, N}}, {{weight, 1}, {neg_offset, N}}, &in));
    MultiNegArgs a = model_args(c, U, V, b, B, N, 0.f);
    a.uid = in.id[0]; a.pid = in.id[1]; a.nid = in.id[2]; a.wt = in.f[0]; a.off = in.f[1];
    return orx_run_forward(c, orx_multineg_nwaves(c, a.D, B), loss_out, l2_out, [&](float* partial) -> int {
        a.partial = partial;
        CHECK(orx_touch_step(U, V, b, a.uid, B, a.pid, B, a.nid, B * N));
        return orx_launch_multineg(c, kind, false, a);
    });
}
