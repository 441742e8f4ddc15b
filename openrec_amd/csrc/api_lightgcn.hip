// LightGCN on the device: orx_lightgcn_create / _destroy / _tables / _propagate / _step / _loss (include/openrec_hip.h has the
// contract, kernels_graph.hip the operator).
//
//   E(0) = [U ; V],  E(k+1) = A~ E(k),  E_f = sum_k alpha_k E(k)
//
// A~ is symmetric and the layer weights are scalars, so dJ/dE(0) = sum_k alpha_k A~^k dJ/dE_f: the backward pass is the forward
// pass on the gradient tables.  One step, all on the context's stream:
//   1. propagate (U, V) -> (Uf, Vf): 2 L half-layers (orx_graph_spmm), the layer sum fused through `acc`
//   2. gather Uf[uid], Vf[pid], Vf[nid]; orx_pair_grads (BPR, no bias, no l2) -> per-occurrence gradients, the loss into an accumulator
//   3. stable sort of the id lists + segmented sums in position order (kernels_rowsort.hip) -> dense GU, GV: no float atomics
//   4. propagate (GU, GV) -> (G0U, G0V)
//   5. the l2 term of the batch's LAYER-0 rows: l2_reg / B * row per occurrence, added into G0U / G0V by the same sorted sums
//   6. the dense optimizer rule on U and V (orx_table_apply_dense's), Adam's counter advanced once
#include "orx_internal.h"
#include "orx_graph.h"

struct orx_lightgcn {
    orx_ctx* ctx = nullptr;
    orx_table* U = nullptr; orx_table* V = nullptr;
    const int64_t* u_ptr = nullptr; const int32_t* u_cols = nullptr;      // user -> items (device)
    const int64_t* i_ptr = nullptr; const int32_t* i_cols = nullptr;      // item -> users (device)
    const float* su = nullptr; const float* sv = nullptr;                 // the two scale vectors (device; NULL: 1)
    int64_t u_long = -1, i_long = -1;                                      // segments of the rows longer than a segment, per CSR (< 0: unknown)
    int L = 0; float alpha[ORX_LIGHTGCN_MAX_LAYERS + 1];
    orx_table* P[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};         // ping-pong layer tables [parity][user, item]
    orx_table* F[2] = {nullptr, nullptr};                                  // Uf, Vf
    orx_table* G[2] = {nullptr, nullptr};                                  // GU, GV: dJ/dE_f
    orx_table* G0[2] = {nullptr, nullptr};                                 // dJ/dE(0)
    // per-batch buffers, grown on demand
    int64_t Bcap = 0;
    int32_t* ids = nullptr;            // [3B] staged uid | pid | nid (host ids)
    int32_t* ids2 = nullptr;           // [2B] pid | nid as one list
    float* rows = nullptr;             // [3B][RS] gathered rows, column D.. stay zero
    float* grads = nullptr;            // [3B][RS] per-occurrence gradients: users, positives, negatives
    float* l2g = nullptr;              // [2B][D]
    uint2* sortU = nullptr; uint2* sortV = nullptr;      // [B], [2B] the sorted (row, position) pairs of the step
    float* partial = nullptr;          // l2 partials
    double* accum = nullptr;           // [4]: (loss, -), (-, l2)
};

static int RS_of(int D) { return (D & ~3) + 4; }

static int lgc_reserve(orx_lightgcn* g, int64_t B) {
    if (B <= g->Bcap) return ORX_OK;
    orx_ctx* c = g->ctx;
    const int D = g->U->dim, RS = RS_of(D);
    ORX_HIP(hipStreamSynchronize(c->stream));
    for (void* p : {(void*)g->ids, (void*)g->ids2, (void*)g->rows, (void*)g->grads, (void*)g->l2g, (void*)g->sortU, (void*)g->sortV, (void*)g->partial}) hipFree(p);
    g->ids = g->ids2 = nullptr; g->rows = g->grads = g->l2g = g->partial = nullptr; g->sortU = g->sortV = nullptr;      // (an allocation below may fail)
    g->Bcap = 0;
    ORX_HIP(hipMalloc((void**)&g->ids, (size_t)3 * B * sizeof(int32_t)));
    ORX_HIP(hipMalloc((void**)&g->ids2, (size_t)2 * B * sizeof(int32_t)));
    ORX_HIP(hipMalloc((void**)&g->rows, (size_t)3 * B * RS * sizeof(float)));
    ORX_HIP(hipMalloc((void**)&g->grads, (size_t)3 * B * RS * sizeof(float)));
    ORX_HIP(hipMalloc((void**)&g->l2g, (size_t)2 * B * D * sizeof(float)));
    ORX_HIP(hipMalloc((void**)&g->sortU, (size_t)B * sizeof(uint2)));
    ORX_HIP(hipMalloc((void**)&g->sortV, (size_t)2 * B * sizeof(uint2)));
    ORX_HIP(hipMalloc((void**)&g->partial, (size_t)orx_graph_l2_nwaves(2 * B) * 2 * sizeof(float)));
    ORX_HIP(hipMemsetAsync(g->rows, 0, (size_t)3 * B * RS * sizeof(float), c->stream));       // (the bias column of orx_pair_grads: zero)
    ORX_HIP(hipMemsetAsync(g->grads, 0, (size_t)3 * B * RS * sizeof(float), c->stream));
    g->Bcap = B;
    return ORX_OK;
}

extern "C" int orx_lightgcn_create(orx_ctx* c, orx_table* user, orx_table* item,
                                   const int64_t* user_ptr, const int32_t* user_cols, const int64_t* item_ptr, const int32_t* item_cols,
                                   const float* user_scale, const float* item_scale, int64_t user_long_segments, int64_t item_long_segments, int32_t layers, const float* layer_weights,
                                   orx_lightgcn** out) {
    static const char* fn = "orx_lightgcn_create";
    ORX_ARG(c && user && item && out, "%s: NULL argument", fn);
    ORX_ARG(user != item && user->w != item->w, "%s: the user and the item table are the same table", fn);
    ORX_ARG(user->ctx == c && item->ctx == c, "%s: the tables live on another context", fn);
    ORX_ARG(user->dim == item->dim, "%s: user dim %d, item dim %d", fn, user->dim, item->dim);
    ORX_ARG(user->dim >= 1 && user->dim <= 128, "%s: dim %d outside [1, 128]", fn, user->dim);
    ORX_ARG(layers >= 1 && layers <= ORX_LIGHTGCN_MAX_LAYERS, "%s: %d layers outside [1, %d]", fn, layers, ORX_LIGHTGCN_MAX_LAYERS);
    ORX_ARG(user_ptr && user_cols && item_ptr && item_cols, "%s: NULL CSR", fn);
    ORX_ARG((user_scale == nullptr) == (item_scale == nullptr), "%s: one scale vector without the other", fn);
    ORX_HIP(hipSetDevice(c->device));
    orx_lightgcn* g = new orx_lightgcn();
    g->ctx = c; g->U = user; g->V = item;
    g->u_ptr = user_ptr; g->u_cols = user_cols; g->i_ptr = item_ptr; g->i_cols = item_cols; g->su = user_scale; g->sv = item_scale;
    g->u_long = user_long_segments; g->i_long = item_long_segments;
    g->L = layers;
    for (int k = 0; k <= layers; ++k) g->alpha[k] = layer_weights ? layer_weights[k] : 1.0f / (float)(layers + 1);
    int rc = ORX_OK;
    for (int side = 0; side < 2 && rc == ORX_OK; ++side) {
        const int64_t rows = side ? item->rows : user->rows;
        for (orx_table** t : {&g->P[0][side], &g->P[1][side], &g->F[side], &g->G[side], &g->G0[side]})
            if (rc == ORX_OK) rc = orx_table_create(c, rows, user->dim, t);
    }
    if (rc == ORX_OK) { hipError_t e = hipMalloc((void**)&g->accum, 4 * sizeof(double)); if (e != hipSuccess) { orx_set_error("%s: hipMalloc failed", fn); rc = ORX_ERR_OOM; } }
    if (rc != ORX_OK) { orx_lightgcn_destroy(g); return rc; }
    *out = g;
    return ORX_OK;
}

extern "C" int orx_lightgcn_destroy(orx_lightgcn* g) {
    if (!g) return ORX_OK;
    hipSetDevice(g->ctx->device);
    hipStreamSynchronize(g->ctx->stream);
    for (int side = 0; side < 2; ++side)
        for (orx_table* t : {g->P[0][side], g->P[1][side], g->F[side], g->G[side], g->G0[side]}) orx_table_destroy(t);
    for (void* p : {(void*)g->ids, (void*)g->ids2, (void*)g->rows, (void*)g->grads, (void*)g->l2g, (void*)g->sortU, (void*)g->sortV, (void*)g->partial, (void*)g->accum}) hipFree(p);
    delete g;
    return ORX_OK;
}

extern "C" int orx_lightgcn_tables(orx_lightgcn* g, orx_table** user_final, orx_table** item_final) {
    ORX_ARG(g && user_final && item_final, "orx_lightgcn_tables: NULL argument");
    *user_final = g->F[0]; *item_final = g->F[1];
    return ORX_OK;
}

// (inU, inV) -> (accU, accV) = sum_k alpha_k A~^k (inU, inV); the layer tables are scratch
static int lgc_propagate(orx_lightgcn* g, orx_table* inU, orx_table* inV, orx_table* accU, orx_table* accV) {
    orx_ctx* c = g->ctx;
    CHECK(orx_table_sync(inU)); CHECK(orx_table_sync(inV));
    CHECK(orx_launch_graph_scale(c, inU->w, accU->w, inU->rows * inU->dim, g->alpha[0]));
    CHECK(orx_launch_graph_scale(c, inV->w, accV->w, inV->rows * inV->dim, g->alpha[0]));
    accU->version++; accV->version++;
    orx_table* cu = inU; orx_table* cv = inV;
    for (int k = 0; k < g->L; ++k) {
        orx_table* nu = g->P[k & 1][0]; orx_table* nv = g->P[k & 1][1];
        CHECK(orx_graph_spmm(c, cv, nu, accU, g->alpha[k + 1], g->u_ptr, g->u_cols, g->su, g->sv, 0, nu->rows, g->u_long, ORX_IDS_DEVICE));
        CHECK(orx_graph_spmm(c, cu, nv, accV, g->alpha[k + 1], g->i_ptr, g->i_cols, g->sv, g->su, 0, nv->rows, g->i_long, ORX_IDS_DEVICE));
        cu = nu; cv = nv;
    }
    return ORX_OK;
}

extern "C" int orx_lightgcn_propagate(orx_lightgcn* g) {
    ORX_ARG(g, "orx_lightgcn_propagate: NULL workspace");
    ORX_HIP(hipSetDevice(g->ctx->device));
    return lgc_propagate(g, g->U, g->V, g->F[0], g->F[1]);
}

static int lgc_ids(orx_lightgcn* g, const int32_t* uid, const int32_t* pid, const int32_t* nid, int64_t B, int flags,
                   const int32_t** du, const int32_t** dp, const int32_t** dn) {
    if (flags & ORX_IDS_DEVICE) { *du = uid; *dp = pid; *dn = nid; return ORX_OK; }
    hipStream_t s = g->ctx->stream;
    ORX_HIP(hipMemcpyAsync(g->ids, uid, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
    ORX_HIP(hipMemcpyAsync(g->ids + B, pid, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
    ORX_HIP(hipMemcpyAsync(g->ids + 2 * B, nid, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
    *du = g->ids; *dp = g->ids + B; *dn = g->ids + 2 * B;
    return ORX_OK;
}

// stages 1 and 2: propagate, gather, the per-occurrence gradients of the batch into g->grads, the loss into accum[0] (the four
// accumulators are zeroed here), pid | nid as one list into g->ids2.  The l2 term is lgc_l2's.
static int lgc_forward(orx_lightgcn* g, const int32_t* du, const int32_t* dp, const int32_t* dn, int64_t B) {
    orx_ctx* c = g->ctx;
    const int D = g->U->dim, RS = RS_of(D);
    CHECK(lgc_propagate(g, g->U, g->V, g->F[0], g->F[1]));
    float* ru = g->rows; float* rp = ru + (size_t)B * RS; float* rn = rp + (size_t)B * RS;
    CHECK(orx_gather_rows(c, g->F[0], nullptr, du, B, ru, RS));
    CHECK(orx_gather_rows(c, g->F[1], nullptr, dp, B, rp, RS));
    CHECK(orx_gather_rows(c, g->F[1], nullptr, dn, B, rn, RS));
    ORX_HIP(hipMemsetAsync(g->accum, 0, 4 * sizeof(double), c->stream));
    float* gu = g->grads; float* gp = gu + (size_t)B * RS; float* gn = gp + (size_t)B * RS;
    CHECK(orx_pair_grads(c, ORX_BPR, D, ru, rp, rn, RS, nullptr, B, B, 0.f, ORX_NO_L2, gu, gp, gn, RS, g->accum));
    CHECK(orx_launch_graph_concat_ids(c, dp, dn, B, g->ids2));
    return ORX_OK;
}

// the l2 term of one table's batch rows: its loss into accum[2..3], its gradient rows (grads != NULL) summed into G0 through `sorted`
static int lgc_l2(orx_lightgcn* g, orx_table* W, const int32_t* ids, int64_t n, float coef, bool grads, const uint2* sorted, orx_table* G0) {
    orx_ctx* c = g->ctx;
    CHECK(orx_launch_graph_l2_rows(c, W->w, W->rows, W->dim, ids, n, coef, grads ? g->l2g : nullptr, g->partial));
    CHECK(orx_launch_loss_accumulate(c, g->partial, orx_graph_l2_nwaves(n), g->accum + 2));
    if (grads) CHECK(orx_csr_accum_into(c, G0->w, G0->rows, G0->dim, sorted, n, g->l2g, W->dim));
    return ORX_OK;
}

static int lgc_fetch(orx_lightgcn* g, float* loss_out, float* l2_out) {
    if (!loss_out && !l2_out) return ORX_OK;
    double h[4];
    ORX_HIP(hipMemcpyAsync(h, g->accum, sizeof(h), hipMemcpyDeviceToHost, g->ctx->stream));
    ORX_HIP(hipStreamSynchronize(g->ctx->stream));
    if (loss_out) *loss_out = (float)h[0];
    if (l2_out) *l2_out = (float)h[3];
    return ORX_OK;
}

static int lgc_check(const char* fn, orx_lightgcn* g, const int32_t* uid, const int32_t* pid, const int32_t* nid, int64_t B, float l2_reg, int flags) {
    ORX_ARG(g, "%s: NULL workspace", fn);
    ORX_ARG(B >= 0 && B < (1LL << 30), "%s: B = %lld out of range", fn, (long long)B);
    ORX_ARG(B == 0 || (uid && pid && nid), "%s: NULL ids", fn);
    ORX_ARG((flags & ~ORX_IDS_DEVICE) == 0, "%s: unknown flags 0x%x", fn, flags);
    ORX_ARG(std::isfinite(l2_reg) && l2_reg >= 0.f, "%s: l2_reg must be finite and >= 0, got %g", fn, (double)l2_reg);
    return ORX_OK;
}

extern "C" int orx_lightgcn_loss(orx_lightgcn* g, const int32_t* uid, const int32_t* pid, const int32_t* nid, int64_t B, float l2_reg,
                                 int flags, float* loss_out, float* l2_out) {
    CHECK(lgc_check("orx_lightgcn_loss", g, uid, pid, nid, B, l2_reg, flags));
    if (B == 0) { if (loss_out) *loss_out = 0.f; if (l2_out) *l2_out = 0.f; return ORX_OK; }
    orx_ctx* c = g->ctx;
    ORX_HIP(hipSetDevice(c->device));
    CHECK(lgc_reserve(g, B));
    const int32_t *du, *dp, *dn;
    CHECK(lgc_ids(g, uid, pid, nid, B, flags, &du, &dp, &dn));
    CHECK(lgc_forward(g, du, dp, dn, B));
    if (l2_reg > 0.f) {
        CHECK(lgc_l2(g, g->U, du, B, l2_reg / (float)B, false, nullptr, nullptr));
        CHECK(lgc_l2(g, g->V, g->ids2, 2 * B, l2_reg / (float)B, false, nullptr, nullptr));
    }
    CHECK(lgc_fetch(g, loss_out, l2_out));
    if (!(flags & ORX_IDS_DEVICE)) return orx_check_index_error(c);
    return ORX_OK;
}

// ---- the dense optimizer apply (orx_table_apply_dense; step 6 here and VBPR's projection, api_vbpr.hip, call the _at form) ----
// the rule on one table at the step the optimizer's counter stands at.  The caller has finished a lazily-applied Adam on the table
// (orx_table_sync: every row current at the step before, the table has left the lazy set) and only then advanced the counter.
int orx_table_apply_dense_at(orx_ctx* c, orx_opt* opt, orx_table* t, const float* grad) {
    OptSlots st;
    CHECK(orx_opt_slots(opt, t, &st));
    float lr = opt->lr, eps = orx_rule_eps(opt), b1 = 0.f, b2 = 0.f;
    if (opt->kind == ORX_ADAM) {
        CHECK(orx_adam_lrt(opt, opt->t));
        lr = opt->h_lrt[(size_t)opt->t]; b1 = opt->p0; b2 = opt->p1; eps = opt->p2;
    }
    CHECK(orx_launch_apply_dense(c, opt->kind, t->w, st.s0, st.s1, grad, t->rows * t->dim, lr, eps, b1, b2));
    t->version++;
    return ORX_OK;
}

extern "C" int orx_table_apply_dense(orx_ctx* c, orx_opt* opt, orx_table* t, const float* grad) {
    static const char* fn = "orx_table_apply_dense";
    ORX_ARG(c && opt && t && grad, "%s: NULL argument", fn);
    ORX_ARG(t->ctx == c && opt->ctx == c, "%s: the table or the optimizer lives on another context", fn);
    ORX_ARG(opt->kind == ORX_SGD || opt->kind == ORX_MOMENTUM || opt->kind == ORX_ADAGRAD || opt->kind == ORX_ADAM,
            "%s: unknown optimizer kind %d", fn, opt->kind);
    ORX_ARG(opt->kind != ORX_ADAM || opt->t + 1 < 0x7fffffff, "%s: step counter overflow", fn);
    ORX_HIP(hipSetDevice(c->device));
    CHECK(orx_table_sync(t));                              // (lazy under this or another optimizer: every row current first)
    if (opt->kind == ORX_ADAM) {
        CHECK(orx_opt_isolate(opt, &t, 1));                // (a shared optimizer: see orx_opt_isolate)
        opt->t += 1;
    }
    return orx_table_apply_dense_at(c, opt, t, grad);
}

extern "C" int orx_lightgcn_step(orx_lightgcn* g, orx_opt* opt, const int32_t* uid, const int32_t* pid, const int32_t* nid, int64_t B,
                                 float l2_reg, int train_mask, int flags, float* loss_out, float* l2_out) {
    static const char* fn = "orx_lightgcn_step";
    CHECK(lgc_check(fn, g, uid, pid, nid, B, l2_reg, flags));
    ORX_ARG(opt && opt->ctx == g->ctx, "%s: NULL optimizer, or one of another context", fn);
    ORX_ARG(opt->kind == ORX_SGD || opt->kind == ORX_MOMENTUM || opt->kind == ORX_ADAGRAD || opt->kind == ORX_ADAM, "%s: unknown optimizer kind %d", fn, opt->kind);
    ORX_ARG((train_mask & ~(ORX_TRAIN_USER | ORX_TRAIN_ITEM)) == 0, "%s: train_mask 0x%x names a table the model does not have", fn, train_mask);
    ORX_ARG(opt->kind != ORX_ADAM || opt->t + 1 < 0x7fffffff, "%s: step counter overflow", fn);
    if (train_mask == 0) train_mask = ORX_TRAIN_USER | ORX_TRAIN_ITEM;
    if (B == 0) return ORX_OK;
    orx_ctx* c = g->ctx;
    const int D = g->U->dim, RS = RS_of(D);
    const bool tu = (train_mask & ORX_TRAIN_USER) != 0, ti = (train_mask & ORX_TRAIN_ITEM) != 0;
    ORX_HIP(hipSetDevice(c->device));
    CHECK(lgc_reserve(g, B));
    const int32_t *du, *dp, *dn;
    CHECK(lgc_ids(g, uid, pid, nid, B, flags, &du, &dp, &dn));
    CHECK(lgc_forward(g, du, dp, dn, B));                              // 1, 2

    // 3. per-occurrence gradients -> dense GU, GV (sorted, summed in position order)
    const float* gu = g->grads; const float* gp = gu + (size_t)B * RS;
    ORX_HIP(hipMemsetAsync(g->G[0]->w, 0, (size_t)g->G[0]->rows * D * sizeof(float), c->stream));
    ORX_HIP(hipMemsetAsync(g->G[1]->w, 0, (size_t)g->G[1]->rows * D * sizeof(float), c->stream));
    CHECK(orx_rows_sort_keep(c, du, 1, B, B, g->U->rows, g->sortU));
    CHECK(orx_rows_sort_keep(c, g->ids2, 1, 2 * B, 2 * B, g->V->rows, g->sortV));
    CHECK(orx_csr_accum_into(c, g->G[0]->w, g->G[0]->rows, D, g->sortU, B, gu, RS));
    CHECK(orx_csr_accum_into(c, g->G[1]->w, g->G[1]->rows, D, g->sortV, 2 * B, gp, RS));
    g->G[0]->version++; g->G[1]->version++;

    CHECK(lgc_propagate(g, g->G[0], g->G[1], g->G0[0], g->G0[1]));            // 4

    if (l2_reg > 0.f) {                                                        // 5
        CHECK(lgc_l2(g, g->U, du, B, l2_reg / (float)B, tu, g->sortU, g->G0[0]));
        CHECK(lgc_l2(g, g->V, g->ids2, 2 * B, l2_reg / (float)B, ti, g->sortV, g->G0[1]));
    }

    // 6. (the tables were brought up to date by the propagation; Adam's counter advances once per step, whatever the mask)
    if (opt->kind == ORX_ADAM) {
        CHECK(orx_table_sync(g->U)); CHECK(orx_table_sync(g->V));
        orx_table* mine[2] = {g->U, g->V};
        CHECK(orx_opt_isolate(opt, mine, 2));
        opt->t += 1;
    }
    if (tu) CHECK(orx_table_apply_dense_at(c, opt, g->U, g->G0[0]->w));
    if (ti) CHECK(orx_table_apply_dense_at(c, opt, g->V, g->G0[1]->w));
    CHECK(lgc_fetch(g, loss_out, l2_out));
    if (!(flags & ORX_IDS_DEVICE)) return orx_check_index_error(c);
    return ORX_OK;
}
