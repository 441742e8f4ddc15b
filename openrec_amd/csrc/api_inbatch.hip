// C-ABI entry points of the in-batch softmax: orx_inbatch_step, orx_inbatch_loss and orx_inbatch_geometry
// (include/openrec_hip.h has the semantics, kernels_inbatch.hip the kernels).
//
// Per step: the touch of (uid; pid), the forward (gather, LSE pass, finalize), the gradient pass (two walks, finish), [Adam: the
// counter advances], then orx_apply_rows of the user table with uid and of the item table and the bias with pid.  No kernel of
// the forward or the gradient pass writes a table, so every gradient is taken on the pre-step tables.  The scratch of a step --
// O(B D chunks) floats, no B x B buffer -- is carved from the context's grow-only d_tmp and reused by every step.
#include <cmath>
#include <cstring>

#include "orx_internal.h"

namespace {

constexpr int IB_FLAGS = ORX_IDS_DEVICE | ORX_NO_L2 | ORX_IB_MASK_HITS | ORX_HOGWILD | ORX_CENSOR;

// what the step and the forward check beyond the shared checks
int check_own(const char* fn, orx_table* U, float scale, int32_t chunk_cols) {
    ORX_ARG(U->dim <= 256, "%s: dim %d above 256", fn, U->dim);
    ORX_ARG(std::isfinite(scale) && scale > 0.f, "%s: scale must be finite and > 0 (got %g)", fn, (double)scale);
    ORX_ARG(chunk_cols >= 0 && chunk_cols % 64 == 0, "%s: chunk_cols must be 0 or a positive multiple of the tile width 64 (got %d)", fn, chunk_cols);
    return ORX_OK;
}

// the step-independent part of the kernels' arguments; grads: with the buffers of the gradient pass
int make_args(orx_ctx* c, orx_table* U, orx_table* V, orx_table* b, int64_t B, float scale, float l2w, int32_t chunk_cols, int flags,
              bool grads, InBatchArgs* out) {
    int32_t geo[4];
    int tpc = 1;
    orx_inbatch_plan(B, U->dim, chunk_cols, geo, &tpc);
    InBatchArgs a;
    memset(&a, 0, sizeof(a));
    a.U = U->w; a.V = V->w; a.b = b ? b->w : nullptr;
    a.B = B; a.Bp = (B + 63) & ~(int64_t)63; a.NU = U->rows; a.NI = V->rows;
    a.D = U->dim; a.Dp = geo[3]; a.gs = (a.D + 1 + 3) & ~3; a.nch = geo[2];
    a.tpc = tpc;
    a.mask = (flags & ORX_IB_MASK_HITS) ? 1 : 0;
    a.scale = scale; a.invB = 1.0f / (float)B; a.l2w = l2w; a.err = c->d_err;
    const size_t row = (size_t)a.Bp * sizeof(float), rows = (size_t)a.Bp * a.Dp * sizeof(float);
    Carve cv;
    const size_t o_xu = cv.take(rows), o_xv = cv.take(rows);
    const size_t o_key = cv.take(row), o_cb = cv.take(row), o_co = cv.take(row), o_cw = cv.take(row), o_sq = cv.take(row);
    const size_t o_pm = cv.take(row * a.nch), o_pe = cv.take(row * a.nch), o_psd = cv.take(row * a.nch);
    const size_t o_rm = cv.take(row), o_cn = cv.take(row), o_dc = cv.take(row), o_rl = cv.take(row);
    size_t o_gpu = 0, o_gpv = 0, o_bp = 0, o_gu = 0, o_gi = 0;
    if (grads) {
        o_gpu = cv.take(rows * a.nch); o_gpv = cv.take(rows * a.nch); o_bp = cv.take(row * a.nch);
        o_gu = cv.take((size_t)B * a.gs * sizeof(float)); o_gi = cv.take((size_t)B * a.gs * sizeof(float));
    }
    ENSURE(c->d_tmp, c->d_tmp_cap, cv.off);
    char* base = reinterpret_cast<char*>(c->d_tmp);
    auto f = [&](size_t o) { return reinterpret_cast<float*>(base + o); };
    a.xu = f(o_xu); a.xv = f(o_xv);
    a.key = reinterpret_cast<int32_t*>(base + o_key); a.cb = f(o_cb); a.co = f(o_co); a.cw = f(o_cw); a.sq = f(o_sq);
    a.pm = f(o_pm); a.pe = f(o_pe); a.psd = f(o_psd); a.rmax = f(o_rm); a.cn = f(o_cn); a.dcoef = f(o_dc); a.rowloss = f(o_rl);
    if (grads) { a.gpu = f(o_gpu); a.gpv = f(o_gpv); a.bpart = f(o_bp); a.gu = f(o_gu); a.gi = f(o_gi); }
    *out = a;
    return ORX_OK;
}

}  // namespace

extern "C" int orx_inbatch_geometry(int64_t B, int32_t D, int32_t chunk_cols, int32_t out[4]) {
    static const char* fn = "orx_inbatch_geometry";
    ORX_ARG(out, "%s: NULL out", fn);
    ORX_ARG(B >= 0 && B <= 0x7fffff00LL, "%s: B = %lld", fn, (long long)B);
    ORX_ARG(D >= 1 && D <= 256, "%s: D must be in [1, 256], got %d", fn, D);
    ORX_ARG(chunk_cols >= 0 && chunk_cols % 64 == 0, "%s: chunk_cols must be 0 or a positive multiple of the tile width 64 (got %d)", fn, chunk_cols);
    orx_inbatch_plan(B, D, chunk_cols, out);
    return ORX_OK;
}

extern "C" int orx_inbatch_step(orx_ctx* c, orx_opt* opt, orx_table* U, orx_table* V, orx_table* b,
                                const int32_t* uid, const int32_t* pid, const float* weight, const float* item_offset,
                                int64_t K, int64_t B, int64_t id_stride, float scale, float l2_reg, int32_t chunk_cols, int flags,
                                float* loss_out, float* l2_out) {
    static const char* fn = "orx_inbatch_step";
    CHECK(orx_check_dot_step(fn, c, opt, U, V, b, 0, K, B, id_stride, l2_reg, flags, IB_FLAGS));
    CHECK(check_own(fn, U, scale, chunk_cols));
    if (K == 0 || B == 0) return ORX_OK;
    ORX_ARG(uid && pid, "%s: NULL id pointer", fn);
    ORX_ARG(B <= 0x7fffff00LL, "%s: B must fit 31 bits", fn);
    ORX_HIP(hipSetDevice(c->device));

    StepInputs in;
    CHECK(orx_stage_steps(c, K, B, id_stride, flags, {{uid, 1}, {pid, 1}}, {{weight, 1}, {item_offset, 1}}, &in));
    InBatchArgs a;
    CHECK(make_args(c, U, V, b, B, scale, l2_reg, chunk_cols, flags, true, &a));
    orx_table* tabs[3] = {U, V, b};
    const int ntabs = b ? 3 : 2;

    return orx_run_steps(c, K, orx_inbatch_npartials(B), flags, loss_out, l2_out, nullptr, [&](int64_t s, int64_t, float* partial) -> int {
        a.uid = in.id[0] + s * in.ds; a.pid = in.id[1] + s * in.ds;
        a.wt = in.f[0] ? in.f[0] + s * in.ds : nullptr;
        a.off = in.f[1] ? in.f[1] + s * in.ds : nullptr;
        a.partial = partial;
        CHECK(orx_touch_step(U, V, b, a.uid, B, a.pid, B, nullptr, 0));
        CHECK(orx_launch_inbatch_forward(c, a));
        CHECK(orx_launch_inbatch_grads(c, a));
        if (opt->kind == ORX_ADAM) CHECK(orx_opt_advance(opt, tabs, ntabs));      // once per step: after the step's reads, before its applies
        CHECK(orx_apply_rows(c, opt, U, nullptr, a.uid, B, a.gu, a.gs));
        return orx_apply_rows(c, opt, V, b, a.pid, B, a.gi, a.gs);
    });
}

extern "C" int orx_inbatch_loss(orx_ctx* c, orx_table* U, orx_table* V, orx_table* b,
                                const int32_t* uid, const int32_t* pid, const float* weight, const float* item_offset,
                                int64_t B, float scale, int32_t chunk_cols, int flags, float* loss_out, float* l2_out, float* row_loss_out) {
    static const char* fn = "orx_inbatch_loss";
    CHECK(orx_check_dot_model(fn, c, U, V, b, 0, flags, IB_FLAGS));
    CHECK(check_own(fn, U, scale, chunk_cols));
    ORX_ARG(!(flags & ORX_NO_L2), "%s: ORX_NO_L2 belongs to the step (the forward has no objective)", fn);
    ORX_ARG(B >= 0 && B <= 0x7fffff00LL, "%s: B = %lld", fn, (long long)B);
    if (B == 0) {
        if (loss_out) *loss_out = 0.f;
        if (l2_out) *l2_out = 0.f;
        return ORX_OK;
    }
    ORX_ARG(uid && pid, "%s: NULL id pointer", fn);
    ORX_HIP(hipSetDevice(c->device));
    StepInputs in;
    CHECK(orx_stage_steps(c, 1, B, B, flags, {{uid, 1}, {pid, 1}}, {{weight, 1}, {item_offset, 1}}, &in));
    InBatchArgs a;
    CHECK(make_args(c, U, V, b, B, scale, 0.f, chunk_cols, flags, false, &a));
    a.uid = in.id[0]; a.pid = in.id[1]; a.wt = in.f[0]; a.off = in.f[1];
    return orx_run_forward(c, orx_inbatch_npartials(B), loss_out, l2_out, [&](float* partial) -> int {
        a.partial = partial;
        CHECK(orx_touch_step(U, V, b, a.uid, B, a.pid, B, nullptr, 0));
        CHECK(orx_launch_inbatch_forward(c, a));
        if (row_loss_out)
            ORX_HIP(hipMemcpyAsync(row_loss_out, a.rowloss, (size_t)B * sizeof(float),
                                   (flags & ORX_IDS_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
        return ORX_OK;
    });
}
