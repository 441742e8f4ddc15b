// C-ABI entry points of the in-batch softmax: orx_inbatch_step, orx_inbatch_loss and orx_inbatch_geometry
// (include/openrec_hip.h has the semantics, kernels_inbatch.hip the kernels).
//
// Per step, all on the context's stream: [lazy Adam: the rows the step reads are replayed to the optimizer's step -- the user
// table with uid, the item table and the bias with pid], the forward (gather, LSE pass, finalize), the gradient pass (two walks,
// finish), [Adam: the counter advances], then orx_apply_rows of the user table with uid and of the item table and the bias with
// pid.  No kernel of the forward or the gradient pass writes a table, so every gradient is taken on the pre-step tables.  The
// loss partials of up to IB_CHUNK steps are summed by one loss_reduce launch, as api_multineg.hip does it.  The scratch of a step
// -- O(B D chunks) floats, no B x B buffer -- is carved from the context's grow-only d_tmp and reused by every step.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "orx_internal.h"

namespace {

constexpr int64_t IB_CHUNK = 32;              // steps whose loss partials are summed by one launch
constexpr int IB_FLAGS = ORX_IDS_DEVICE | ORX_NO_L2 | ORX_IB_MASK_HITS | ORX_HOGWILD | ORX_CENSOR;

struct Carve {                                // consecutive 256-byte aligned pieces of one device buffer
    size_t off = 0;
    size_t take(size_t bytes) { const size_t at = off; off += (bytes + 255) & ~(size_t)255; return at; }
};

// what the step and the forward share
int check_model(const char* fn, orx_ctx* c, orx_table* U, orx_table* V, orx_table* b, float scale, int32_t chunk_cols, int flags) {
    ORX_ARG(c && U && V, "%s: NULL context/table", fn);
    ORX_ARG(U->ctx == c && V->ctx == c && (!b || b->ctx == c), "%s: the tables belong to a different context", fn);
    ORX_ARG(U->dim == V->dim, "%s: user dim %d != item dim %d (dot scores only)", fn, U->dim, V->dim);
    ORX_ARG(U->dim <= 256, "%s: dim %d above 256", fn, U->dim);
    ORX_ARG(!b || (b->dim == 1 && b->rows == V->rows), "%s: item_bias must be [%lld, 1]", fn, (long long)V->rows);
    ORX_ARG(std::isfinite(scale) && scale > 0.f, "%s: scale must be finite and > 0 (got %g)", fn, (double)scale);
    ORX_ARG(chunk_cols >= 0 && chunk_cols % 64 == 0, "%s: chunk_cols must be 0 or a positive multiple of the tile width 64 (got %d)", fn, chunk_cols);
    ORX_ARG((flags & ~IB_FLAGS) == 0, "%s: unknown flags", fn);
    ORX_ARG(!(flags & ORX_HOGWILD), "%s: ORX_HOGWILD is a speed-comparison mode of the plain pairwise step only", fn);
    ORX_ARG(!(flags & ORX_CENSOR), "%s: ORX_CENSOR belongs to UCML; this step scores by dot products only (UCML / L2 scoring is not offered)", fn);
    return ORX_OK;
}

// the inputs of K steps on the device: arrays that are there already as they are (stride ds = id_stride), host arrays packed at
// stride B into the context's staging buffers (ids: d_ids, weights and offsets: d_lab)
struct Inputs { const int32_t* du; const int32_t* dp; const float* dw; const float* doff; int64_t ds; };

int stage_inputs(orx_ctx* c, const int32_t* uid, const int32_t* pid, const float* weight, const float* off,
                 int64_t K, int64_t B, int64_t id_stride, int flags, Inputs* in) {
    if (flags & ORX_IDS_DEVICE) { *in = Inputs{uid, pid, weight, off, id_stride}; return ORX_OK; }
    const int64_t n = K * B;
    ENSURE(c->d_ids, c->d_ids_cap, (size_t)n * 2 * sizeof(int32_t));
    if (weight || off) ENSURE(c->d_lab, c->d_lab_cap, (size_t)n * 2 * sizeof(float));
    for (int64_t s = 0; s < K; ++s) {
        CHECK(stage_ids(c, uid + s * id_stride, B, s * B));
        CHECK(stage_ids(c, pid + s * id_stride, B, n + s * B));
        if (weight) ORX_HIP(hipMemcpyAsync(c->d_lab + s * B, weight + s * id_stride, (size_t)B * sizeof(float), hipMemcpyHostToDevice, c->stream));
        if (off) ORX_HIP(hipMemcpyAsync(c->d_lab + n + s * B, off + s * id_stride, (size_t)B * sizeof(float), hipMemcpyHostToDevice, c->stream));
    }
    *in = Inputs{c->d_ids, c->d_ids + n, weight ? c->d_lab : nullptr, off ? c->d_lab + n : nullptr, B};
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
    ORX_ARG(opt, "%s: NULL optimizer", fn);
    CHECK(check_model(fn, c, U, V, b, scale, chunk_cols, flags));
    ORX_ARG(opt->ctx == c, "%s: the optimizer belongs to a different context", fn);
    ORX_ARG(std::isfinite(l2_reg) && l2_reg >= 0.f, "%s: l2_reg must be finite and >= 0 (got %g)", fn, (double)l2_reg);
    ORX_ARG(!(flags & ORX_NO_L2) || l2_reg == 0.f, "%s: ORX_NO_L2 together with l2_reg = %g (drop the flag, or pass l2_reg = 0)", fn, (double)l2_reg);
    ORX_ARG(K >= 0 && B >= 0 && id_stride >= 0, "%s: negative K, B or id_stride", fn);
    // what orx_apply_rows would refuse for this optimizer and these tables, with its message, before anything is launched
    ORX_ARG(opt->kind == ORX_SGD || opt->kind == ORX_ADAGRAD || opt->kind == ORX_MOMENTUM || (opt->kind == ORX_ADAM && (!b || orx_adam_rows_lazy(opt, V))),
            "orx_apply_rows: the whole-table-sweep form of Adam (ORX_ADAM_DENSE) takes no bias column");
    if (K == 0 || B == 0) return ORX_OK;
    ORX_ARG(uid && pid, "%s: NULL id pointer", fn);
    ORX_ARG(K == 1 || id_stride >= B, "%s: id_stride %lld below B = %lld", fn, (long long)id_stride, (long long)B);
    ORX_ARG(B <= 0x7fffff00LL, "%s: B must fit 31 bits", fn);
    const bool adam = opt->kind == ORX_ADAM;
    ORX_ARG(!adam || opt->t + K < 0x7fffffff, "%s: step counter overflow", fn);
    ORX_HIP(hipSetDevice(c->device));

    Inputs in;
    CHECK(stage_inputs(c, uid, pid, weight, item_offset, K, B, id_stride, flags, &in));
    InBatchArgs a;
    CHECK(make_args(c, U, V, b, B, scale, l2_reg, chunk_cols, flags, true, &a));
    const int np = orx_inbatch_npartials(B);
    const int64_t chunk = std::min<int64_t>(K, IB_CHUNK);
    const bool want = loss_out != nullptr || l2_out != nullptr;
    ENSURE(c->d_partial, c->d_partial_cap, (size_t)chunk * np * 2 * sizeof(float));
    if (want) ENSURE(c->d_loss, c->d_loss_cap, (size_t)K * 2 * sizeof(double));
    orx_table* tabs[3] = {U, V, b};
    const int ntabs = b ? 3 : 2;

    for (int64_t s0 = 0; s0 < K; s0 += chunk) {
        const int64_t kc = std::min<int64_t>(chunk, K - s0);
        for (int64_t i = 0; i < kc; ++i) {
            const int64_t s = s0 + i;
            a.uid = in.du + s * in.ds; a.pid = in.dp + s * in.ds;
            a.wt = in.dw ? in.dw + s * in.ds : nullptr;
            a.off = in.doff ? in.doff + s * in.ds : nullptr;
            a.partial = c->d_partial + (size_t)i * np * 2;
            // a lazily-applied table: exactly the rows this step reads (no-ops for a table that is current)
            CHECK(orx_table_touch(U, a.uid, B));
            CHECK(orx_table_touch(V, a.pid, B));
            if (b) CHECK(orx_table_touch(b, a.pid, B));
            CHECK(orx_launch_inbatch_forward(c, a));
            CHECK(orx_launch_inbatch_grads(c, a));
            if (adam) CHECK(orx_opt_advance(opt, tabs, ntabs));        // once per step: after the step's reads, before its applies
            CHECK(orx_apply_rows(c, opt, U, nullptr, a.uid, B, a.gu, a.gs));
            CHECK(orx_apply_rows(c, opt, V, b, a.pid, B, a.gi, a.gs));
        }
        if (want) {
            ReduceArgs r;
            r.partial = c->d_partial; r.out = c->d_loss + 2 * s0; r.nwaves = np;
            CHECK(orx_launch_loss_reduce(c, r, kc));
        }
    }
    CHECK(fetch_losses(c, K, loss_out, l2_out));
    if (!(flags & ORX_IDS_DEVICE)) return orx_check_index_error(c);
    return ORX_OK;
}

extern "C" int orx_inbatch_loss(orx_ctx* c, orx_table* U, orx_table* V, orx_table* b,
                                const int32_t* uid, const int32_t* pid, const float* weight, const float* item_offset,
                                int64_t B, float scale, int32_t chunk_cols, int flags, float* loss_out, float* l2_out, float* row_loss_out) {
    static const char* fn = "orx_inbatch_loss";
    CHECK(check_model(fn, c, U, V, b, scale, chunk_cols, flags));
    ORX_ARG(!(flags & ORX_NO_L2), "%s: ORX_NO_L2 belongs to the step (the forward has no objective)", fn);
    ORX_ARG(B >= 0 && B <= 0x7fffff00LL, "%s: B = %lld", fn, (long long)B);
    if (B == 0) {
        if (loss_out) *loss_out = 0.f;
        if (l2_out) *l2_out = 0.f;
        return ORX_OK;
    }
    ORX_ARG(uid && pid, "%s: NULL id pointer", fn);
    ORX_HIP(hipSetDevice(c->device));
    Inputs in;
    CHECK(stage_inputs(c, uid, pid, weight, item_offset, 1, B, B, flags, &in));
    InBatchArgs a;
    CHECK(make_args(c, U, V, b, B, scale, 0.f, chunk_cols, flags, false, &a));
    const int np = orx_inbatch_npartials(B);
    ENSURE(c->d_partial, c->d_partial_cap, (size_t)np * 2 * sizeof(float));
    ENSURE(c->d_loss, c->d_loss_cap, 2 * sizeof(double));
    a.uid = in.du; a.pid = in.dp; a.wt = in.dw; a.off = in.doff; a.partial = c->d_partial;
    CHECK(orx_table_touch(U, a.uid, B));
    CHECK(orx_table_touch(V, a.pid, B));
    if (b) CHECK(orx_table_touch(b, a.pid, B));
    CHECK(orx_launch_inbatch_forward(c, a));
    ReduceArgs r;
    r.partial = c->d_partial; r.out = c->d_loss; r.nwaves = np;
    CHECK(orx_launch_loss_reduce(c, r, 1));
    if (row_loss_out)
        ORX_HIP(hipMemcpyAsync(row_loss_out, a.rowloss, (size_t)B * sizeof(float),
                               (flags & ORX_IDS_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    float dummy;
    CHECK(fetch_losses(c, 1, loss_out ? loss_out : &dummy, l2_out));
    return orx_check_index_error(c);
}
