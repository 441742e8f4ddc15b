// C-ABI entry points of the partial train step: orx_pairwise_step_subset / orx_pointwise_step_subset (include/openrec_hip.h has
// the semantics).  A mask that names every table is the full step itself; a strict subset takes the route below.
//
// Per chunk of steps: the id lists of the trained tables are sorted once for all steps of the chunk (kernels_rowsort.hip, one
// launch set with grid.y = step; the item table and the bias share one sort of the concatenated positive | negative ids).  Per
// step: [lazy Adam: the rows the step reads from a trained table are replayed to the optimizer's step], ONE gradient launch
// (kernels_subset.hip) that writes gradient rows for the trained roles only, then orx_apply_rows_sorted of every trained table,
// all four optimizer kinds.  The gradient launch ends before the applies begin, so every gradient is taken on the pre-step
// tables.  Frozen tables are arguments of the gradient launch alone, as const pointers; no optimizer slot is looked up for them.
#include <algorithm>
#include <cstring>

#include "orx_internal.h"

namespace {

constexpr int ORX_TRAIN_ALL = ORX_TRAIN_USER | ORX_TRAIN_ITEM | ORX_TRAIN_BIAS;

// the mask checks both entry points share; *full: the mask names every table the call was given
int check_mask(const char* fn, int mask, const orx_table* bias, bool* full) {
    ORX_ARG(mask != 0, "%s: empty train mask (no table would be trained)", fn);
    ORX_ARG((mask & ~ORX_TRAIN_ALL) == 0, "%s: train mask 0x%x has bits outside ORX_TRAIN_USER | ORX_TRAIN_ITEM | ORX_TRAIN_BIAS", fn, mask);
    ORX_ARG(bias != nullptr || !(mask & ORX_TRAIN_BIAS), "%s: ORX_TRAIN_BIAS without a bias table (bias is NULL)", fn);
    *full = mask == (bias ? ORX_TRAIN_ALL : (ORX_TRAIN_USER | ORX_TRAIN_ITEM));
    return ORX_OK;
}

// one trained table of a step
struct Trained { orx_table* t; const uint2* sorted; int64_t n; float* grads; int64_t g_stride; };

// what the two models have in common: everything but the gradient launch's model arguments
struct SubsetCall {
    orx_ctx* c; orx_opt* opt; orx_table* U; orx_table* V; orx_table* b;
    int mask; int kmodel;                     // orx_launch_subset_grads' model
    int refs;                                 // item lookups per sample: 2 (pairwise: positive, negative) or 1 (WRMF)
    int flags;
    StepInputs in;                            // id: uid, pid / iid, nid (pairwise)
    const float* dl; const float* dw;         // of in.f: WRMF's labels; pairwise: per-triplet weights, NULL: all ones
    int64_t K, B;
    SubsetArgs a;                             // model constants filled in by the caller
};

int run_subset(SubsetCall& q, float* loss_out, float* l2_out) {
    orx_ctx* c = q.c; orx_opt* opt = q.opt;
    const int64_t K = q.K, B = q.B, nI = q.refs * B, ds = q.in.ds;
    const int32_t* du = q.in.id[0]; const int32_t* di = q.in.id[1]; const int32_t* dn = q.in.id[2];
    const int D = q.U->dim;
    const bool tU = (q.mask & ORX_TRAIN_USER) != 0, tV = (q.mask & ORX_TRAIN_ITEM) != 0, tb = (q.mask & ORX_TRAIN_BIAS) != 0;
    const bool adam = opt->kind == ORX_ADAM;
    ORX_ARG(!adam || opt->t + K < 0x7fffffff, "train step: step counter overflow");
    // frozen tables: finished under the old counter (whatever optimizer they are lazy under), then only read; the same for
    // any other table lazy under `opt` (orx_opt_isolate).  Trained tables stay lazy under `opt` where they are.
    orx_table* keep[3]; int n_keep = 0;
    if (tU) keep[n_keep++] = q.U;
    if (tV) keep[n_keep++] = q.V;
    if (tb) keep[n_keep++] = q.b;
    if (!tU) CHECK(orx_table_sync(q.U));
    if (!tV) CHECK(orx_table_sync(q.V));
    if (!tb && q.b) CHECK(orx_table_sync(q.b));
    CHECK(orx_opt_isolate(opt, keep, n_keep));
    for (int i = 0; i < n_keep; ++i)
        if (!(adam && orx_adam_rows_lazy(opt, keep[i]) && keep[i]->lazy == opt)) CHECK(orx_table_sync(keep[i]));
    if (adam) CHECK(orx_adam_lrt(opt, opt->t + K + 1));

    // scratch, one buffer: sorted lists of the chunk, the concatenated item ids, one step's gradient rows
    const int64_t chunk = std::min<int64_t>(K, ORX_STEP_CHUNK);
    Carve cv;
    const size_t o_su = cv.take(tU ? (size_t)chunk * B * sizeof(uint2) : 0);
    const size_t o_si = cv.take((tV || tb) ? (size_t)chunk * nI * sizeof(uint2) : 0);
    const size_t o_ci = cv.take(((tV || tb) && q.refs == 2) ? (size_t)chunk * nI * sizeof(int32_t) : 0);
    const size_t o_gu = cv.take(tU ? (size_t)B * D * sizeof(float) : 0);
    const size_t o_gi = cv.take(tV ? (size_t)nI * D * sizeof(float) : 0);
    const size_t o_gb = cv.take(tb ? (size_t)nI * sizeof(float) : 0);
    ENSURE(c->d_tmp, c->d_tmp_cap, cv.off);
    char* base = reinterpret_cast<char*>(c->d_tmp);
    uint2* sortU = reinterpret_cast<uint2*>(base + o_su);
    uint2* sortI = reinterpret_cast<uint2*>(base + o_si);
    int32_t* catI = reinterpret_cast<int32_t*>(base + o_ci);
    SubsetArgs a = q.a;
    a.U = q.U->w; a.V = q.V->w; a.b = q.b ? q.b->w : nullptr;
    a.gu = tU ? reinterpret_cast<float*>(base + o_gu) : nullptr;
    a.gi = tV ? reinterpret_cast<float*>(base + o_gi) : nullptr;
    a.gb = tb ? reinterpret_cast<float*>(base + o_gb) : nullptr;
    a.B = B; a.NU = q.U->rows; a.NI = q.V->rows; a.D = D; a.err = c->d_err;

    auto sort_chunk = [&](int64_t s0, int64_t kc) -> int {
        if (tV || tb) {
            const int32_t* ids = di + s0 * ds; int64_t stride = ds;
            if (q.refs == 2) {
                CHECK(orx_launch_subset_concat_ids(c, di + s0 * ds, dn + s0 * ds, ds, kc, B, catI));
                ids = catI; stride = nI;
            }
            CHECK(orx_rows_sort_keep(c, ids, kc, nI, stride, q.V->rows, sortI));
        }
        if (tU) CHECK(orx_rows_sort_keep(c, du + s0 * ds, kc, B, ds, q.U->rows, sortU));
        return ORX_OK;
    };
    return orx_run_steps(c, K, orx_fused_nwaves(D, B), q.flags, loss_out, l2_out, sort_chunk, [&](int64_t s, int64_t i, float* partial) -> int {
        Trained tr[3]; int nt = 0;
        if (tU) tr[nt++] = Trained{q.U, sortU + i * B, B, a.gu, D};
        if (tV) tr[nt++] = Trained{q.V, sortI + i * nI, nI, a.gi, D};
        if (tb) tr[nt++] = Trained{q.b, sortI + i * nI, nI, a.gb, 1};
        // lazy Adam: the rows of a trained table this step reads are brought to the optimizer's present step first
        if (adam)
            for (int k = 0; k < nt; ++k)
                if (tr[k].t->lazy == opt) CHECK(orx_adam_rows_sorted(c, opt, tr[k].t, tr[k].sorted, tr[k].n, nullptr, 0, false));
        a.uid = du + s * ds; a.pid = di + s * ds; a.nid = dn ? dn + s * ds : nullptr;
        a.label = q.dl ? q.dl + s * ds : nullptr;
        a.wt = q.dw ? q.dw + s * ds : nullptr;
        a.partial = partial;
        CHECK(orx_launch_subset_grads(c, q.kmodel, a));
        if (adam) opt->t += 1;                // once per step, whatever the mask
        for (int k = 0; k < nt; ++k) CHECK(orx_apply_rows_sorted(c, opt, tr[k].t, tr[k].sorted, tr[k].n, tr[k].grads, tr[k].g_stride));
        return ORX_OK;
    });
}

}  // namespace

extern "C" int orx_pairwise_step_subset(orx_ctx* c, int model, orx_opt* opt, orx_table* U, orx_table* V, orx_table* b,
                                        const int32_t* uid, const int32_t* pid, const int32_t* nid,
                                        int64_t K, int64_t B, int64_t id_stride, float margin, int flags,
                                        int train_mask, float* loss_out, float* l2_out) {
    return orx_pairwise_subset_impl(c, model, opt, U, V, b, uid, pid, nid, nullptr, K, B, id_stride, margin, (flags & ORX_NO_L2) ? 0.f : 1.f, flags,
                                    train_mask, loss_out, l2_out);
}

// (weight, l2w: as orx_pairwise_step_impl)
int orx_pairwise_subset_impl(orx_ctx* c, int model, orx_opt* opt, orx_table* U, orx_table* V, orx_table* b,
                             const int32_t* uid, const int32_t* pid, const int32_t* nid, const float* weight,
                             int64_t K, int64_t B, int64_t id_stride, float margin, float l2w, int flags,
                             int train_mask, float* loss_out, float* l2_out) {
    bool full = false;
    CHECK(check_mask("orx_pairwise_step_subset", train_mask, b, &full));
    // the full mask, and the calls that touch no table (K = 0, an empty batch), are the full step's: its checks, its route
    if (full || K <= 0 || B <= 0) return orx_pairwise_step_impl(c, model, opt, U, V, b, uid, pid, nid, weight, K, B, id_stride, margin, l2w, flags, loss_out, l2_out);
    ORX_ARG(!(flags & ORX_HOGWILD), "orx_pairwise_step_subset: ORX_HOGWILD trains every table (a strict subset is not supported with it)");
    ORX_ARG(!(flags & ORX_CENSOR), "orx_pairwise_step_subset: ORX_CENSOR is not folded into a step over a strict subset (call orx_table_censor after it)");
    ORX_ARG(c && opt, "orx_pairwise_step_subset: NULL context/optimizer");
    ORX_ARG(model == ORX_BPR || model == ORX_UCML, "orx_pairwise_step_subset: unknown model %d", model);
    ORX_ARG(U && V, "orx_pairwise_step_subset: NULL table");
    ORX_ARG(b || model != ORX_UCML, "orx_pairwise_step_subset: UCML needs the item bias table (bias may be NULL with ORX_BPR only)");
    ORX_ARG(U->ctx == c && V->ctx == c && (!b || b->ctx == c) && opt->ctx == c, "orx_pairwise_step_subset: objects belong to a different context");
    ORX_ARG(U->dim == V->dim, "orx_pairwise_step_subset: user dim %d != item dim %d", U->dim, V->dim);
    ORX_ARG(!b || (b->dim == 1 && b->rows == V->rows), "orx_pairwise_step_subset: item_bias must be [%lld, 1]", (long long)V->rows);
    ORX_ARG(U->dim <= 256, "orx_pairwise_step_subset: dims up to 256 (got %d)", U->dim);
    ORX_ARG(uid && pid && nid, "orx_pairwise_step_subset: NULL id pointer");
    ORX_HIP(hipSetDevice(c->device));
    SubsetCall q;
    memset(&q, 0, sizeof(q));
    q.c = c; q.opt = opt; q.U = U; q.V = V; q.b = b; q.mask = train_mask; q.kmodel = b ? model : MODEL_BPR_NB; q.refs = 2; q.flags = flags; q.K = K; q.B = B;
    CHECK(orx_stage_steps(c, K, B, id_stride, flags, {{uid, 1}, {pid, 1}, {nid, 1}}, {{weight, 1}}, &q.in));
    q.dw = q.in.f[0];
    q.a.margin = margin; q.a.invB = 1.0f / (float)B; q.a.l2w = l2w;
    return run_subset(q, loss_out, l2_out);
}

extern "C" int orx_pointwise_step_subset(orx_ctx* c, int model, orx_opt* opt, orx_table* U, orx_table* V, orx_table* b, orx_table* w,
                                         const int32_t* uid, const int32_t* iid, const float* label,
                                         int64_t K, int64_t B, int64_t id_stride, float a_w, float b_w, int flags,
                                         int train_mask, float* loss_out, float* l2_out) {
    return orx_pointwise_subset_impl(c, model, opt, U, V, b, w, uid, iid, label, K, B, id_stride, a_w, b_w, (flags & ORX_NO_L2) ? 0.f : 1.f, flags,
                                     train_mask, loss_out, l2_out);
}

int orx_pointwise_subset_impl(orx_ctx* c, int model, orx_opt* opt, orx_table* U, orx_table* V, orx_table* b, orx_table* w,
                              const int32_t* uid, const int32_t* iid, const float* label,
                              int64_t K, int64_t B, int64_t id_stride, float a_w, float b_w, float l2w, int flags,
                              int train_mask, float* loss_out, float* l2_out) {
    bool full = false;
    CHECK(check_mask("orx_pointwise_step_subset", train_mask, b, &full));
    if (full || K <= 0 || B <= 0) return orx_pointwise_step_impl(c, model, opt, U, V, b, w, uid, iid, label, K, B, id_stride, a_w, b_w, l2w, flags, loss_out, l2_out);
    ORX_ARG(model != ORX_GMF, "orx_pointwise_step_subset: ORX_GMF with a strict subset is not supported (its Dense(1) kernel is a fourth role)");
    ORX_ARG(!(flags & ORX_HOGWILD), "orx_pointwise_step_subset: ORX_HOGWILD trains every table (a strict subset is not supported with it)");
    ORX_ARG(c && opt, "orx_pointwise_step_subset: NULL context/optimizer");
    ORX_ARG(model == ORX_WRMF, "orx_pointwise_step_subset: unknown model %d", model);
    ORX_ARG(U && V && b, "orx_pointwise_step_subset: NULL table");
    ORX_ARG(U->ctx == c && V->ctx == c && b->ctx == c && opt->ctx == c, "orx_pointwise_step_subset: objects belong to a different context");
    ORX_ARG(U->dim == V->dim, "orx_pointwise_step_subset: user dim %d != item dim %d", U->dim, V->dim);
    ORX_ARG(b->dim == 1 && b->rows == V->rows, "orx_pointwise_step_subset: item_bias must be [%lld, 1]", (long long)V->rows);
    ORX_ARG(U->dim <= 256, "orx_pointwise_step_subset: dims up to 256 (got %d)", U->dim);
    ORX_ARG(uid && iid && label, "orx_pointwise_step_subset: NULL id/label pointer");
    ORX_HIP(hipSetDevice(c->device));
    SubsetCall q;
    memset(&q, 0, sizeof(q));
    q.c = c; q.opt = opt; q.U = U; q.V = V; q.b = b; q.mask = train_mask; q.kmodel = -1; q.refs = 1; q.flags = flags; q.K = K; q.B = B;
    CHECK(orx_stage_steps(c, K, B, id_stride, flags, {{uid, 1}, {iid, 1}}, {{label, 1}}, &q.in));
    q.dl = q.in.f[0];
    q.a.invB = 1.0f / (float)B; q.a.l2w = l2w; q.a.a_w = a_w; q.a.b_w = b_w;
    q.a.sigmoid = (flags & ORX_POINT_SIGMOID) ? 1 : 0;
    return run_subset(q, loss_out, l2_out);
}
