// C-ABI entry points of VBPR: orx_features_project, orx_vbpr_item_table, orx_vbpr_step, orx_vbpr_loss and orx_vbpr_geometry
// (include/openrec_hip.h has the semantics, kernels_vbpr.hip the kernels).
//
// Per step: the touch of (uid; pid, nid), the projection Delta = (F[pid] - F[nid]) E, the pass over the triplets (gradient rows,
// coefficient rows R, loss partials), the projection gradient dE = df^T R + l2_proj E, [Adam: the counter advances], then
// orx_apply_rows of the user table with uid, of the item table and of the bias with pid | nid, and the dense rule on E at the
// step's count.  No kernel before the applies writes a table, so every gradient is taken on the pre-step tables.  The item table
// and the bias are applied as two tables with the same id list -- orx_apply_rows_sorted on ONE sort of the list, no float atomics
// --, so a table gets the same bits whichever other tables the train mask names.  The scratch of a step is carved from the
// context's grow-only d_tmp and reused by every step.
#include <cmath>
#include <cstring>

#include "orx_graph.h"
#include "orx_internal.h"

namespace {

constexpr int64_t VB_MAX_B = 0x7fffffffLL - 256;
constexpr int VB_TRAIN_ALL = ORX_TRAIN_USER | ORX_TRAIN_ITEM | ORX_TRAIN_BIAS | ORX_TRAIN_PROJ;
constexpr int VB_FLAGS = ORX_IDS_DEVICE | ORX_NO_L2 | ORX_HOGWILD | ORX_CENSOR;

int check_features(const char* fn, orx_ctx* c, const float* F, int64_t NI, int32_t Fd, orx_table* E) {
    ORX_ARG(c && F && E, "%s: NULL context, feature matrix or projection", fn);
    ORX_ARG(E->ctx == c, "%s: the projection belongs to a different context", fn);
    ORX_ARG(NI >= 1 && NI <= 0x7fffffffLL, "%s: %lld feature rows", fn, (long long)NI);
    ORX_ARG(Fd >= 1 && Fd <= 8192, "%s: feature dim Fd must be in [1, 8192], got %d", fn, Fd);
    ORX_ARG(E->rows == Fd, "%s: the projection has %lld rows for features of dim %d", fn, (long long)E->rows, Fd);
    ORX_ARG(E->dim >= 1 && E->dim <= 128, "%s: projection width Dc must be in [1, 128], got %d", fn, E->dim);
    return ORX_OK;
}

int check_chunk(const char* fn, int64_t B, int32_t batch_chunk) {
    ORX_ARG(batch_chunk >= 0 && batch_chunk % 64 == 0, "%s: batch_chunk must be 0 or a positive multiple of 64 (got %d)", fn, batch_chunk);
    ORX_ARG(batch_chunk == 0 || (B + batch_chunk - 1) / batch_chunk <= 65535, "%s: batch_chunk %d makes more than 65535 chunks of B = %lld", fn,
            batch_chunk, (long long)B);
    return ORX_OK;
}

// what the step and the forward check before the shared checks (which then find U->dim == V->dim + E->dim)
int check_own(const char* fn, orx_ctx* c, orx_table* U, orx_table* V, orx_table* E, const float* F, int64_t NI, int32_t Fd,
              int64_t B, int32_t batch_chunk) {
    ORX_ARG(c && U && V, "%s: NULL context/table", fn);
    CHECK(check_features(fn, c, F, NI, Fd, E));
    ORX_ARG(V->dim >= 1, "%s: latent dim %d", fn, V->dim);
    ORX_ARG(V->dim + E->dim <= 256, "%s: D = Dl + Dc = %d + %d above 256", fn, V->dim, E->dim);
    ORX_ARG(U->dim == V->dim + E->dim, "%s: user dim %d != item latent dim %d + projection width %d", fn, U->dim, V->dim, E->dim);
    ORX_ARG(V->rows == NI, "%s: %lld feature rows for %lld items", fn, (long long)NI, (long long)V->rows);
    ORX_ARG(B >= 0 && B < VB_MAX_B, "%s: B = %lld (B < 2^31 - 256)", fn, (long long)B);
    return check_chunk(fn, B, batch_chunk);
}

struct StepArgs { VbprProjArgs pj; VbprPairArgs pa; VbprDprojArgs dp; uint2* sorted; };      // sorted: [2B] the item list's (row, position) pairs

// the step-independent part of the kernels' arguments; grads: with the buffers of the gradient pass
int make_args(orx_ctx* c, orx_table* U, orx_table* V, orx_table* b, orx_table* E, const float* F, int64_t NI, int32_t Fd, int64_t B,
              float l2w, float l2p, int32_t batch_chunk, bool grads, StepArgs* out) {
    const int Dl = V->dim, Dc = E->dim, D = Dl + Dc;
    const int gs = (D + 1 + 3) & ~3;
    int32_t geo[4];
    orx_vbpr_plan(B, Fd, Dc, batch_chunk, geo);
    const int vec = (Fd % 4 == 0 && (uintptr_t)F % 16 == 0) ? 1 : 0;
    Carve cv;
    const size_t o_delta = cv.take((size_t)B * Dc * sizeof(float));
    size_t o_gu = 0, o_gi = 0, o_R = 0, o_list = 0, o_part = 0, o_dE = 0, o_sorted = 0;
    if (grads) {
        o_gu = cv.take((size_t)B * gs * sizeof(float)); o_gi = cv.take((size_t)2 * B * gs * sizeof(float));
        o_R = cv.take((size_t)B * Dc * sizeof(float)); o_list = cv.take((size_t)2 * B * sizeof(int32_t));
        o_part = cv.take((size_t)geo[1] * Fd * Dc * sizeof(float)); o_dE = cv.take((size_t)Fd * Dc * sizeof(float));
        o_sorted = cv.take((size_t)2 * B * sizeof(uint2));
    }
    ENSURE(c->d_tmp, c->d_tmp_cap, cv.off);
    char* base = reinterpret_cast<char*>(c->d_tmp);
    auto f = [&](size_t o) { return reinterpret_cast<float*>(base + o); };
    StepArgs s;
    memset(&s, 0, sizeof(s));
    s.pj.F = F; s.pj.E = E->w; s.pj.row0 = 0; s.pj.n = B; s.pj.NI = NI; s.pj.Fd = Fd; s.pj.Dc = Dc; s.pj.Np = geo[2]; s.pj.vec = vec;
    s.pj.out = f(o_delta); s.pj.out_stride = Dc; s.pj.out_col0 = 0; s.pj.err = c->d_err;
    s.pa.U = U->w; s.pa.V = V->w; s.pa.b = b ? b->w : nullptr; s.pa.delta = f(o_delta);
    s.pa.B = B; s.pa.NU = U->rows; s.pa.NI = NI; s.pa.Dl = Dl; s.pa.Dc = Dc; s.pa.gs = gs;
    s.pa.invB = 1.0f / (float)B; s.pa.l2w = l2w; s.pa.err = c->d_err;
    if (grads) {
        s.pa.gu = f(o_gu); s.pa.gi = f(o_gi); s.pa.R = f(o_R); s.pa.list = reinterpret_cast<int32_t*>(base + o_list);
        s.dp.F = F; s.dp.R = f(o_R); s.dp.B = B; s.dp.NI = NI; s.dp.chunk_rows = geo[0]; s.dp.Fd = Fd; s.dp.Dc = Dc; s.dp.Np = geo[2];
        s.dp.vec = vec; s.dp.nch = geo[1]; s.dp.part = f(o_part); s.dp.E = E->w; s.dp.l2p = l2p; s.dp.dE = f(o_dE);
        s.sorted = reinterpret_cast<uint2*>(base + o_sorted);
    }
    *out = s;
    return ORX_OK;
}

}  // namespace

extern "C" int orx_vbpr_geometry(int64_t B, int32_t Fd, int32_t Dc, int32_t batch_chunk, int32_t out[4]) {
    static const char* fn = "orx_vbpr_geometry";
    ORX_ARG(out, "%s: NULL out", fn);
    ORX_ARG(B >= 0 && B < VB_MAX_B, "%s: B = %lld (B < 2^31 - 256)", fn, (long long)B);
    ORX_ARG(Fd >= 1 && Fd <= 8192, "%s: feature dim Fd must be in [1, 8192], got %d", fn, Fd);
    ORX_ARG(Dc >= 1 && Dc <= 128, "%s: projection width Dc must be in [1, 128], got %d", fn, Dc);
    CHECK(check_chunk(fn, B, batch_chunk));
    orx_vbpr_plan(B, Fd, Dc, batch_chunk, out);
    return ORX_OK;
}

extern "C" int orx_features_project(orx_ctx* c, const float* F, int64_t NI, int32_t Fd, orx_table* E, const int32_t* ia, const int32_t* ib,
                                    int64_t row0, int64_t n, float* out, int64_t out_stride, int32_t out_col0, int flags) {
    static const char* fn = "orx_features_project";
    CHECK(check_features(fn, c, F, NI, Fd, E));
    ORX_ARG((flags & ~ORX_IDS_DEVICE) == 0, "%s: flags other than ORX_IDS_DEVICE", fn);
    ORX_ARG(n >= 0 && n < VB_MAX_B, "%s: n = %lld (n < 2^31 - 256)", fn, (long long)n);
    ORX_ARG(out_col0 >= 0 && out_stride >= (int64_t)out_col0 + E->dim, "%s: columns [%d, %d) do not fit rows of %lld floats", fn, out_col0,
            out_col0 + E->dim, (long long)out_stride);
    ORX_ARG(ia || (row0 >= 0 && row0 + n <= NI), "%s: rows [%lld, %lld) outside the %lld feature rows", fn, (long long)row0, (long long)(row0 + n),
            (long long)NI);
    if (n == 0) return ORX_OK;
    ORX_ARG(out, "%s: NULL output", fn);
    ORX_HIP(hipSetDevice(c->device));
    CHECK(orx_table_sync(E));
    const bool host = !(flags & ORX_IDS_DEVICE) && (ia || ib);
    if (host) {
        ENSURE(c->d_ids, c->d_ids_cap, (size_t)n * 2 * sizeof(int32_t));
        if (ia) { CHECK(stage_ids(c, ia, n, 0)); ia = c->d_ids; }
        if (ib) { CHECK(stage_ids(c, ib, n, n)); ib = c->d_ids + n; }
    }
    VbprProjArgs a;
    memset(&a, 0, sizeof(a));
    a.F = F; a.E = E->w; a.ia = ia; a.ib = ib; a.row0 = row0; a.n = n; a.NI = NI; a.Fd = Fd; a.Dc = E->dim; a.Np = (E->dim + 15) & ~15;
    a.vec = (Fd % 4 == 0 && (uintptr_t)F % 16 == 0) ? 1 : 0;
    a.out = out; a.out_stride = out_stride; a.out_col0 = out_col0; a.err = c->d_err;
    CHECK(orx_launch_vbpr_project(c, a));
    if (host) return orx_check_index_error(c);
    return ORX_OK;
}

extern "C" int orx_vbpr_item_table(orx_ctx* c, orx_table* V, orx_table* E, const float* F, int64_t NI, int32_t Fd, int64_t row0, int64_t nrows,
                                   orx_table* W) {
    static const char* fn = "orx_vbpr_item_table";
    ORX_ARG(V && W, "%s: NULL table", fn);
    CHECK(check_features(fn, c, F, NI, Fd, E));
    ORX_ARG(V->ctx == c && W->ctx == c, "%s: the tables belong to a different context", fn);
    ORX_ARG(V->rows == NI && W->rows == NI, "%s: %lld feature rows, %lld item rows, %lld output rows", fn, (long long)NI, (long long)V->rows,
            (long long)W->rows);
    ORX_ARG(W->dim == V->dim + E->dim && W->w != V->w, "%s: the output must be another table of dim %d + %d", fn, V->dim, E->dim);
    ORX_ARG(row0 >= 0 && nrows >= 0 && row0 + nrows <= NI, "%s: rows [%lld, %lld) outside the %lld items", fn, (long long)row0,
            (long long)(row0 + nrows), (long long)NI);
    if (nrows == 0) return ORX_OK;
    ORX_HIP(hipSetDevice(c->device));
    CHECK(orx_table_sync(V)); CHECK(orx_table_sync(E)); CHECK(orx_table_sync(W));
    const int Dl = V->dim, D = W->dim;
    CHECK(orx_launch_vbpr_copy_cols(c, V->w + (size_t)row0 * Dl, Dl, W->w + (size_t)row0 * D, D, nrows));
    VbprProjArgs a;
    memset(&a, 0, sizeof(a));
    a.F = F; a.E = E->w; a.row0 = row0; a.n = nrows; a.NI = NI; a.Fd = Fd; a.Dc = E->dim; a.Np = (E->dim + 15) & ~15;
    a.vec = (Fd % 4 == 0 && (uintptr_t)F % 16 == 0) ? 1 : 0;
    a.out = W->w + (size_t)row0 * D; a.out_stride = D; a.out_col0 = Dl; a.err = c->d_err;
    CHECK(orx_launch_vbpr_project(c, a));
    W->version++;
    return ORX_OK;
}

extern "C" int orx_vbpr_step(orx_ctx* c, orx_opt* opt, orx_table* U, orx_table* V, orx_table* b, orx_table* E, const float* F, int64_t NI,
                             int32_t Fd, const int32_t* uid, const int32_t* pid, const int32_t* nid, const float* weight,
                             int64_t K, int64_t B, int64_t id_stride, float l2_reg, float l2_proj, int32_t batch_chunk, int train_mask,
                             int flags, float* loss_out, float* l2_out) {
    static const char* fn = "orx_vbpr_step";
    CHECK(check_own(fn, c, U, V, E, F, NI, Fd, B, batch_chunk));
    CHECK(orx_check_dot_step(fn, c, opt, U, V, b, E->dim, K, B, id_stride, l2_reg, flags, VB_FLAGS));
    ORX_ARG(std::isfinite(l2_proj) && l2_proj >= 0.f, "%s: l2_proj must be finite and >= 0 (got %g)", fn, (double)l2_proj);
    ORX_ARG(!(flags & ORX_NO_L2) || l2_proj == 0.f, "%s: ORX_NO_L2 together with l2_proj = %g (drop the flag, or pass 0)", fn, (double)l2_proj);
    ORX_ARG((train_mask & ~VB_TRAIN_ALL) == 0, "%s: train mask 0x%x has bits outside ORX_TRAIN_USER | ORX_TRAIN_ITEM | ORX_TRAIN_BIAS | ORX_TRAIN_PROJ",
            fn, train_mask);
    ORX_ARG(b != nullptr || !(train_mask & ORX_TRAIN_BIAS), "%s: ORX_TRAIN_BIAS without a bias table (bias is NULL)", fn);
    if (train_mask == 0) train_mask = ORX_TRAIN_USER | ORX_TRAIN_ITEM | ORX_TRAIN_PROJ | (b ? ORX_TRAIN_BIAS : 0);
    if (K == 0 || B == 0) return ORX_OK;
    ORX_ARG(uid && pid && nid, "%s: NULL id pointer", fn);
    ORX_HIP(hipSetDevice(c->device));
    const bool tU = (train_mask & ORX_TRAIN_USER) != 0, tV = (train_mask & ORX_TRAIN_ITEM) != 0, tb = (train_mask & ORX_TRAIN_BIAS) != 0,
               tE = (train_mask & ORX_TRAIN_PROJ) != 0;

    StepInputs in;
    CHECK(orx_stage_steps(c, K, B, id_stride, flags, {{uid, 1}, {pid, 1}, {nid, 1}}, {{weight, 1}}, &in));
    StepArgs a;
    CHECK(make_args(c, U, V, b, E, F, NI, Fd, B, l2_reg, l2_proj, batch_chunk, true, &a));
    const int Dl = V->dim, gs = a.pa.gs;
    // a table outside the mask is finished under the old counter (whatever optimizer it is lazy under), then only read; the
    // projection is a dense parameter: every row current before the step reads it
    orx_table* keep[4]; int n_keep = 0;
    if (tU) keep[n_keep++] = U; else CHECK(orx_table_sync(U));
    if (tV) keep[n_keep++] = V; else CHECK(orx_table_sync(V));
    if (b) { if (tb) keep[n_keep++] = b; else CHECK(orx_table_sync(b)); }
    CHECK(orx_table_sync(E));
    if (tE) keep[n_keep++] = E;

    return orx_run_steps(c, K, orx_vbpr_nwaves(c, B), flags, loss_out, l2_out, nullptr, [&](int64_t s, int64_t, float* partial) -> int {
        const int32_t* du = in.id[0] + s * in.ds; const int32_t* dp = in.id[1] + s * in.ds; const int32_t* dn = in.id[2] + s * in.ds;
        a.pj.ia = dp; a.pj.ib = dn;
        a.pa.uid = du; a.pa.pid = dp; a.pa.nid = dn; a.pa.wt = in.f[0] ? in.f[0] + s * in.ds : nullptr;
        a.pa.partial = partial;
        a.dp.pid = dp; a.dp.nid = dn;
        CHECK(orx_touch_step(U, V, b, du, B, dp, B, dn, B));
        CHECK(orx_launch_vbpr_project(c, a.pj));
        CHECK(orx_launch_vbpr_pairs(c, true, a.pa));
        if (tE) CHECK(orx_launch_vbpr_dproj(c, a.dp));
        if (opt->kind == ORX_ADAM) CHECK(orx_opt_advance(opt, keep, n_keep));      // once per step: after the step's reads, before its applies
        if (tU) CHECK(orx_apply_rows(c, opt, U, nullptr, du, B, a.pa.gu, gs));
        if (tV || tb) {                   // one sort of pid | nid for both (kept aside: the user table's apply sorts again)
            CHECK(orx_rows_sort_keep(c, a.pa.list, 1, 2 * B, 2 * B, V->rows, a.sorted));
            if (tV) CHECK(orx_apply_rows_sorted(c, opt, V, a.sorted, 2 * B, a.pa.gi, gs));
            if (tb) CHECK(orx_apply_rows_sorted(c, opt, b, a.sorted, 2 * B, a.pa.gi + Dl, gs));
        }
        if (tE) CHECK(orx_table_apply_dense_at(c, opt, E, a.dp.dE));
        return ORX_OK;
    });
}

extern "C" int orx_vbpr_loss(orx_ctx* c, orx_table* U, orx_table* V, orx_table* b, orx_table* E, const float* F, int64_t NI, int32_t Fd,
                             const int32_t* uid, const int32_t* pid, const int32_t* nid, const float* weight, int64_t B, int flags,
                             float* loss_out, float* l2_out) {
    static const char* fn = "orx_vbpr_loss";
    CHECK(check_own(fn, c, U, V, E, F, NI, Fd, B, 0));
    CHECK(orx_check_dot_model(fn, c, U, V, b, E->dim, flags, VB_FLAGS));
    ORX_ARG(!(flags & ORX_NO_L2), "%s: ORX_NO_L2 belongs to the step (the forward has no objective)", fn);
    if (B == 0) {
        if (loss_out) *loss_out = 0.f;
        if (l2_out) *l2_out = 0.f;
        return ORX_OK;
    }
    ORX_ARG(uid && pid && nid, "%s: NULL id pointer", fn);
    ORX_HIP(hipSetDevice(c->device));
    StepInputs in;
    CHECK(orx_stage_steps(c, 1, B, B, flags, {{uid, 1}, {pid, 1}, {nid, 1}}, {{weight, 1}}, &in));
    StepArgs a;
    CHECK(make_args(c, U, V, b, E, F, NI, Fd, B, 0.f, 0.f, 0, false, &a));
    a.pj.ia = in.id[1]; a.pj.ib = in.id[2];
    a.pa.uid = in.id[0]; a.pa.pid = in.id[1]; a.pa.nid = in.id[2]; a.pa.wt = in.f[0];
    return orx_run_forward(c, orx_vbpr_nwaves(c, B), loss_out, l2_out, [&](float* partial) -> int {
        a.pa.partial = partial;
        CHECK(orx_table_sync(E));
        CHECK(orx_touch_step(U, V, b, a.pa.uid, B, a.pa.pid, B, a.pa.nid, B));
        CHECK(orx_launch_vbpr_project(c, a.pj));
        return orx_launch_vbpr_pairs(c, false, a.pa);
    });
}
