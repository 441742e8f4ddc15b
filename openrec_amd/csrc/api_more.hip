// C-ABI entry points of the pointwise step and its loss and of the sharded building blocks (row gather, pair gradients, the
// applies of gradient rows with lazy Adam and the planned apply, the device-side exchange plan).  The device sampler's are in
// api_sampler.hip.
#include <vector>
#include <cmath>
#include <cstring>

#include "orx_internal.h"

// ------------------------------------------------------------ pointwise step ---
static int check_point_tables(int model, orx_table* U, orx_table* V, orx_table* b, orx_table* w) {
    ORX_ARG(model == ORX_GMF || model == ORX_WRMF, "pointwise: unknown model %d", model);
    ORX_ARG(U && V && b, "pointwise: NULL table");
    ORX_ARG(U->dim == V->dim, "pointwise: user dim %d != item dim %d", U->dim, V->dim);
    ORX_ARG(b->dim == 1 && b->rows == V->rows, "pointwise: item_bias must be [%lld, 1]", (long long)V->rows);
    ORX_ARG(model != ORX_GMF || (w && w->rows == U->dim && w->dim == 1), "pointwise: GMF needs the Dense kernel w as a [D, 1] table");
    return ORX_OK;
}

extern "C" int orx_pointwise_step(orx_ctx* c, int model, orx_opt* opt,
                                  orx_table* U, orx_table* V, orx_table* b, orx_table* w,
                                  const int32_t* uid, const int32_t* iid, const float* label,
                                  int64_t K, int64_t B, int64_t id_stride, float a_w, float b_w, int flags,
                                  float* loss_out, float* l2_out) {
    return orx_pointwise_step_impl(c, model, opt, U, V, b, w, uid, iid, label, K, B, id_stride, a_w, b_w, (flags & ORX_NO_L2) ? 0.f : 1.f, flags,
                                   loss_out, l2_out);
}

// (l2w: the coefficient of l2_loss in the objective -- orx_pointwise_step_l2reg; the plain entry point passes 0 or 1)
int orx_pointwise_step_impl(orx_ctx* c, int model, orx_opt* opt, orx_table* U, orx_table* V, orx_table* b, orx_table* w,
                            const int32_t* uid, const int32_t* iid, const float* label,
                            int64_t K, int64_t B, int64_t id_stride, float a_w, float b_w, float l2w, int flags,
                            float* loss_out, float* l2_out) {
    ORX_ARG(c && opt, "orx_pointwise_step: NULL context/optimizer");
    CHECK(check_point_tables(model, U, V, b, w));
    ORX_ARG(K >= 0 && B > 0, "orx_pointwise_step: K must be >= 0 and B > 0");
    ORX_ARG(K == 0 || (uid && iid && label), "orx_pointwise_step: NULL id/label pointer");
    if (K == 0) return ORX_OK;
    ORX_HIP(hipSetDevice(c->device));
    StepInputs in;
    CHECK(orx_stage_steps(c, K, B, id_stride, flags, {{uid, 1}, {iid, 1}}, {{label, 1}}, &in));
    const int32_t *du = in.id[0], *di = in.id[1]; const float* dl = in.f[0]; const int64_t ds = in.ds;
    const bool hogwild = (flags & ORX_HOGWILD) != 0;
    ORX_ARG(!hogwild || opt->kind != ORX_MOMENTUM, "orx_pointwise_step: ORX_HOGWILD is not supported with momentum (its racy in-place pass has no velocity rule)");
    const int fb = orx_fallback_bits();
    // TF-2.0 Adam applied lazily, as in orx_pairwise_step: float4 dims with the exact-step plan; the
    // Dense(1) kernel of GMF is a dense parameter and takes the plain rule.  Otherwise every reference accumulates
    // and the tables are swept whole.
    const bool lazy_adam = opt->kind == ORX_ADAM && !hogwild && orx_fused_can_inline_apply(U->dim) && U->rows < (1LL << 28) &&
                           V->rows < (1LL << 28) && !(fb & 1) && U->owned && V->owned && b->owned && getenv("ORX_ADAM_DENSE") == nullptr;
    const int mode = (opt->kind == ORX_ADAM && !lazy_adam) ? MODE_ACCUM : (hogwild ? MODE_HOGWILD : MODE_EXACT);
    const bool lazy_resume = lazy_adam && U->lazy == opt && V->lazy == opt && b->lazy == opt;
    if (!lazy_resume) for (orx_table* t : {U, V, b}) CHECK(orx_table_sync(t));
    { orx_table* mine[3] = {U, V, b}; CHECK(orx_opt_isolate(opt, mine, 3)); }      // (a shared optimizer: api.hip orx_opt_isolate)
    if (w) CHECK(orx_table_sync(w));
    CHECK(orx_table_scratch(U)); CHECK(orx_table_scratch(V)); CHECK(orx_table_scratch(b));
    if (w) CHECK(orx_table_scratch(w));
    OptSlots sU, sV, sb, sw;
    CHECK(orx_opt_slots(opt, U, &sU)); CHECK(orx_opt_slots(opt, V, &sV)); CHECK(orx_opt_slots(opt, b, &sb));
    if (w) CHECK(orx_opt_slots(opt, w, &sw));
    const int D = U->dim;
    const int nw = orx_point_nwaves(D, B);
    const int nslot = nw + (model == ORX_GMF ? 1 : 0);      // + one slot for 0.5*||w||^2
    ENSURE(c->d_partial, c->d_partial_cap, (size_t)K * nslot * 2 * sizeof(float));
    ENSURE(c->d_loss, c->d_loss_cap, (size_t)K * 2 * sizeof(double));
    if (model == ORX_GMF) ENSURE(c->d_wpart, c->d_wpart_cap, (size_t)(nw + 256) * D * sizeof(float));   // + stage-1 rows of dense_reduce
    const int64_t list_stride = 2 * B;
    // exact mode on the float4 dims below 2^28 rows: the plan of the pairwise step (roles: rows referenced twice get
    // plain stores; staging plan + reduction tree for hot rows), made once for all K steps.  Otherwise byte flags +
    // atomics for every duplicate.
    const bool role_bits = mode == MODE_EXACT && orx_fused_can_inline_apply(D) && U->rows < (1LL << 28) && V->rows < (1LL << 28) && !(fb & 1);
    const bool staging = role_bits && !(fb & 8);
    // the previous step's duplicated rows are applied by extra blocks of the next step's launch, as in the pairwise step
    // (WRMF 27.1 -> see DESIGN 4.4; fb bit 2: separate dup_apply launches)
    const bool inline_apply = role_bits && K > 1 && orx_plan_v2(true) && !(fb & 2);
    PairPlan plan;
    memset(&plan, 0, sizeof(plan));
    if (role_bits) {
        CHECK(orx_table_scratch(U, true)); CHECK(orx_table_scratch(V, true)); CHECK(orx_table_scratch(b, true));
        const int nb_total = orx_dedup_buckets(U->rows) + orx_dedup_buckets(V->rows);
        CHECK(orx_exact_buffers(c, U, V, K, B, mode, true, inline_apply, staging, nb_total, nslot, &plan));
        if (opt->kind == ORX_ADAM) plan.min_late = 1;      // Adam: fixed summation order for every row referenced >= 3 times (api.hip)
        // pairing (round 6): as in orx_pairwise_step -- SGD, float4 dims with >= 2 samples per wavefront, paused for 32 calls when a plan
        // accepts few pairs.  ORX_NO_PAIR=1 / ORX_POINT_NO_PAIR=1 / ORX_FORCE_FALLBACK bit 4: off
        if (orx_pairing_wanted(mode, true, opt->kind, D, B, fb) && getenv("ORX_POINT_NO_PAIR") == nullptr) {
            if (c->pair_pause > 0) c->pair_pause -= 1;
            else CHECK(orx_pairing_buffers(c, B, D, &plan));
        }
        ENSURE(c->d_partial, c->d_partial_cap, (size_t)K * nslot * 2 * sizeof(float));      // (orx_exact_buffers sized it for its own shape: a chunk)
    } else if (mode == MODE_EXACT) {
        ENSURE(c->d_dflag, c->d_dflag_cap, (size_t)K * 2 * B);
        ENSURE(c->d_dlist, c->d_dlist_cap, (size_t)K * list_stride * sizeof(uint32_t));
        ENSURE(c->d_dcount, c->d_dcount_cap, (size_t)K * sizeof(int));
        DedupArgs d;
        memset(&d, 0, sizeof(d));
        d.uid = du; d.pid = di; d.nid = di; d.id_stride = ds;
        d.dflag = c->d_dflag; d.dlist = c->d_dlist; d.dcount = c->d_dcount;
        d.flag_stride = 2 * B; d.list_stride = list_stride;
        d.nU = B; d.nP = B; d.nN = 0; d.NU = U->rows; d.NI = V->rows;
        d.nbu = orx_dedup_buckets(U->rows); d.nbi = orx_dedup_buckets(V->rows);
        ORX_HIP(hipMemsetAsync(c->d_dcount, 0, (size_t)K * sizeof(int), c->stream));
        CHECK(orx_launch_dedup(c, d, K));
    }
    PointArgs a;
    memset(&a, 0, sizeof(a));
    a.U = U->w; a.V = V->w; a.b = b->w; a.w = w ? w->w : nullptr;
    a.gU = U->gsum; a.gV = V->gsum; a.gb = b->gsum;
    a.aU = sU.s0; a.aV = sV.s0; a.ab = sb.s0;
    a.B = B; a.NU = U->rows; a.NI = V->rows; a.D = D;
    a.lr = opt->lr; a.eps = orx_rule_eps(opt);
    a.invB = 1.0f / (float)B; a.l2w = l2w; a.a_w = a_w; a.b_w = b_w;
    a.sigmoid = (model == ORX_WRMF && (flags & ORX_POINT_SIGMOID)) ? 1 : 0;
    a.wpartial = c->d_wpart; a.err = c->d_err;
    // GMF on the float4 kernels: the Dense(1) gradient is reduced and applied by the last workgroups of the step's own launch
    const bool dense_tail = model == ORX_GMF && orx_point_dense_tail_ok(D);
    if (dense_tail) {
        // the partial rows and the group rows behind them start out EMPTY (all ones); every launch hands them back that way
        const size_t nrows = (size_t)orx_point_wparts(D, B) + (size_t)orx_point_reducers(D, B) - 1;
        ORX_HIP(hipMemsetAsync(c->d_wpart, 0xff, nrows * D * sizeof(float), c->stream));
        a.wt_nred = orx_point_reducers(D, B); a.wt_rows = c->d_wpart + (size_t)orx_point_wparts(D, B) * D;
        const bool to_gout = mode == MODE_ACCUM || lazy_adam;                        // (Adam: adam_sweep_kernel applies the gradient)
        a.wt_gout = to_gout ? w->gsum : nullptr; a.wt_acc = to_gout ? nullptr : sw.s0; a.wt_optkind = to_gout ? -1 : opt->kind;
    }
    if (role_bits) { a.role_bits = 1; a.gU2 = U->gsum2; a.gV2 = V->gsum2; a.gb2 = b->gsum2; a.readyU = U->ready; a.readyV = V->ready; }
    PairArgs pa;                                 // view of the same tables for dup_apply_kernel / hot_reduce_kernel / the in-launch apply
    memset(&pa, 0, sizeof(pa));
    pa.U = U->w; pa.V = V->w; pa.b = b->w; pa.gU = U->gsum; pa.gV = V->gsum; pa.gb = b->gsum;
    if (role_bits) { pa.gU2 = U->gsum2; pa.gV2 = V->gsum2; pa.gb2 = b->gsum2; pa.role_bits = 1; pa.readyU = U->ready; pa.readyV = V->ready; }
    CHECK(orx_epochs_reserve(c, K, {U, V}));      // epochs tag the ready flags: one per step
    pa.aU = sU.s0; pa.aV = sV.s0; pa.ab = sb.s0; pa.B = B; pa.D = D; pa.lr = a.lr; pa.eps = a.eps;
    if (lazy_adam) {
        CHECK(orx_lazy_adam_fill(opt, U, V, b, sU, sV, sb, !lazy_resume, K, &a));
        // (the view for dup_apply_kernel / the in-launch apply: the same, but its replay loops)
        pa.a2U = a.a2U; pa.a2V = a.a2V; pa.a2b = a.a2b; pa.lastU = a.lastU; pa.lastV = a.lastV; pa.lastb = a.lastb;
        pa.lrt = a.lrt; pa.b1 = a.b1; pa.b2 = a.b2; pa.eps = a.eps; pa.newton = a.newton;
    }
    const int64_t chunk = role_bits ? plan.chunk : K;
    for (int64_t s0 = 0; s0 < K; s0 += chunk) {
    const int64_t kc = (K - s0 < chunk) ? (K - s0) : chunk;
    ExactChunk ck;
    if (role_bits) {
        c->plan_label = plan.pair_tpw > 1 ? dl + s0 * ds : nullptr;
        const int rc_plan = orx_exact_plan_chunk(c, U, V, du + s0 * ds, di + s0 * ds, di + s0 * ds, ds, B, B, 0, kc, B, true, inline_apply, staging, plan, &ck);
        c->plan_label = nullptr;
        CHECK(rc_plan);
    }
    const bool inl = inline_apply && !ck.hot && !ck.dense_dups;      // (many duplicated rows / reduction-tree levels: separate launches, api.hip)
    for (int64_t i = 0; i < kc; ++i) {
        const int64_t s = s0 + i;
        a.label = dl + s * ds;
        a.partial = c->d_partial + (size_t)s * nslot * 2;
        a.wt_l2slot = a.partial + 2 * nw;
        if (role_bits) {
            a.uid = c->d_ids2 + (size_t)i * 3 * plan.Bp; a.iid = a.uid + plan.Bp;
            a.ids4 = plan.pair_tpw > 1 ? c->d_ids4 + (size_t)i * B : nullptr;      // (with pairing the SoA copy is not written: the records are the input)
            orx_exact_step_views(c, plan, i, B, D, ck.use_stage, &pa);
            a.refinfo = pa.refinfo; a.segstart = pa.segstart; a.stage = pa.stage; a.stageb = pa.stageb;
        } else {
            a.uid = du + s * ds; a.iid = di + s * ds;
            a.dflag = c->d_dflag + (size_t)s * 2 * B;
            pa.dlist = c->d_dlist + (size_t)s * list_stride; pa.dcount = c->d_dcount + s;
        }
        if (lazy_adam) { opt->t += 1; a.step_t = pa.step_t = (int)opt->t; }
        a.n_apply_blocks = 0;
        if (role_bits) {
            a.epoch = pa.epoch = ++c->epoch;
            if (inl && i > 0) {                  // this launch also applies the duplicated rows of step i-1
                pa.n_apply_blocks = orx_apply_blocks(B, D);
                pa.prev_dlist = c->d_dlist + (size_t)(i - 1) * plan.list_stride; pa.prev_dcount = c->d_dcount + (i - 1);
                a.n_apply_blocks = pa.n_apply_blocks;
                a.ap = pa;
            }
        }
        CHECK(orx_launch_point_fused(c, model, opt->kind, mode, a));
        if (mode == MODE_EXACT) {
            for (int l = 0; l < ck.tree_levels; ++l) CHECK(orx_launch_hot_reduce(c, pa, l));
            if (!inl || i == kc - 1) CHECK(orx_launch_dup_apply(c, opt->kind, pa));
        }
        float lr_t = lazy_adam ? opt->h_lrt[(size_t)opt->t] : 0.f;
        if (mode == MODE_ACCUM) CHECK(orx_adam_dense_step(c, opt, {{U, sU}, {V, sV}, {b, sb}}, &lr_t));
        if (model == ORX_GMF) {                  // dense Dense(1) kernel: reduce partials, apply the dense rule
            if (mode == MODE_ACCUM || lazy_adam) {
                if (!dense_tail) CHECK(orx_launch_dense_reduce(c, c->d_wpart, orx_point_wparts(D, B), D, w->w, a.l2w, w->gsum, a.partial + 2 * nw, nullptr, -1, 0.f, 0.f));
                CHECK(orx_launch_adam_sweep(c, w->w, sw.s0, sw.s1, w->gsum, D, lr_t, opt->p0, opt->p1, opt->p2));
            } else if (!dense_tail) {        // reduce + dense SGD / Adagrad rule in one launch
                CHECK(orx_launch_dense_reduce(c, c->d_wpart, orx_point_wparts(D, B), D, w->w, a.l2w, nullptr, a.partial + 2 * nw, sw.s0, opt->kind, opt->lr, a.eps));
            }
        }
    }
    }
    ReduceArgs r;
    r.partial = c->d_partial; r.out = c->d_loss; r.nwaves = nslot;
    CHECK(orx_launch_loss_reduce(c, r, K));
    CHECK(fetch_losses(c, K, loss_out, l2_out));
    if (!(flags & ORX_IDS_DEVICE)) return orx_check_index_error(c);
    return ORX_OK;
}

extern "C" int orx_pointwise_loss(orx_ctx* c, int model, orx_table* U, orx_table* V, orx_table* b, orx_table* w,
                                  const int32_t* uid, const int32_t* iid, const float* label,
                                  int64_t B, float a_w, float b_w, int flags, float* loss_out, float* l2_out) {
    if (U) CHECK(orx_table_sync(U));
    if (V) CHECK(orx_table_sync(V));
    if (b) CHECK(orx_table_sync(b));
    if (w) CHECK(orx_table_sync(w));
    ORX_ARG(c, "orx_pointwise_loss: NULL context");
    CHECK(check_point_tables(model, U, V, b, w));
    ORX_ARG(B > 0 && uid && iid && label, "orx_pointwise_loss: empty batch or NULL pointer");
    ORX_HIP(hipSetDevice(c->device));
    StepInputs in;
    CHECK(orx_stage_steps(c, 1, B, B, flags, {{uid, 1}, {iid, 1}}, {{label, 1}}, &in));
    const int D = U->dim;
    const int nw = orx_point_nwaves(D, B);
    const int nslot = nw + (model == ORX_GMF ? 1 : 0);
    ENSURE(c->d_partial, c->d_partial_cap, (size_t)nslot * 2 * sizeof(float));
    ENSURE(c->d_loss, c->d_loss_cap, 2 * sizeof(double));
    PointArgs a;
    memset(&a, 0, sizeof(a));
    a.U = U->w; a.V = V->w; a.b = b->w; a.w = w ? w->w : nullptr;
    a.B = B; a.NU = U->rows; a.NI = V->rows; a.D = D;
    a.invB = 1.0f / (float)B; a.l2w = 1.f; a.a_w = a_w; a.b_w = b_w;
    a.sigmoid = (model == ORX_WRMF && (flags & ORX_POINT_SIGMOID)) ? 1 : 0;
    a.partial = c->d_partial; a.err = c->d_err;
    a.uid = in.id[0]; a.iid = in.id[1]; a.label = in.f[0];
    CHECK(orx_launch_point_fused(c, model, ORX_SGD, MODE_LOSS, a));
    if (model == ORX_GMF) CHECK(orx_launch_dense_reduce(c, nullptr, 0, D, w->w, 0.f, nullptr, c->d_partial + 2 * nw, nullptr, -1, 0.f, 0.f));
    ReduceArgs r;
    r.partial = c->d_partial; r.out = c->d_loss; r.nwaves = nslot;
    CHECK(orx_launch_loss_reduce(c, r, 1));
    CHECK(fetch_losses(c, 1, loss_out, l2_out));
    return orx_check_index_error(c);
}

extern "C" int orx_gather_rows(orx_ctx* ctx, orx_table* t, orx_table* bias, const int32_t* ids, int64_t n,
                               float* out, int64_t out_stride) {
    if (t) CHECK(orx_table_touch(t, ids, n));            // a lazy table: only the rows read are brought up to date
    if (bias) CHECK(orx_table_touch(bias, ids, n));
    ORX_ARG(ctx && t && (n == 0 || (ids && out)), "orx_gather_rows: NULL argument");
    ORX_ARG(out_stride >= t->dim + (bias ? 1 : 0), "orx_gather_rows: out_stride %lld too small", (long long)out_stride);
    ORX_HIP(hipSetDevice(ctx->device));
    return orx_launch_gather(ctx, t->w, bias ? bias->w : nullptr, t->rows, t->dim, ids, n, out, out_stride, ctx->d_err, 1);
}

extern "C" int orx_pair_grads(orx_ctx* ctx, int model, int32_t D,
                              const float* u_rows, const float* p_rows, const float* n_rows, int64_t row_stride,
                              const int32_t* valid, int64_t T, int64_t B_global, float margin, int flags,
                              float* gu, float* gp, float* gn, int64_t g_stride, double* loss_l2_accum) {
    ORX_ARG(ctx && u_rows && p_rows && n_rows && gu && gp && gn, "orx_pair_grads: NULL argument");
    ORX_ARG(model == ORX_BPR || model == ORX_UCML, "orx_pair_grads: unknown model %d", model);
    ORX_ARG(D > 0 && row_stride > D && g_stride > D, "orx_pair_grads: strides must leave room for the bias column");
    ORX_ARG(B_global > 0, "orx_pair_grads: B_global must be positive");
    if (T == 0) return ORX_OK;
    ORX_HIP(hipSetDevice(ctx->device));
    GradArgs a;
    memset(&a, 0, sizeof(a));
    a.u = u_rows; a.p = p_rows; a.n = n_rows; a.row_stride = row_stride; a.valid = valid;
    a.gu = gu; a.gp = gp; a.gn = gn; a.g_stride = g_stride;
    a.T = T; a.D = D; a.invB = 1.0f / (float)B_global; a.margin = margin;
    a.l2w = (flags & ORX_NO_L2) ? 0.f : 1.f;
    // upper bound of the wave count (one lane group per triplet, 4 waves per block)
    ENSURE(ctx->d_partial, ctx->d_partial_cap, (size_t)(T + 4) * 2 * sizeof(float));
    a.partial = ctx->d_partial;
    int nw = 0;
    CHECK(orx_launch_pair_grads(ctx, model, a, &nw));
    if (loss_l2_accum) CHECK(orx_launch_loss_accumulate(ctx, ctx->d_partial, nw, loss_l2_accum));
    return ORX_OK;
}

// ---- lazy TF-2.0 Adam on gradient rows -------------------------------------------------------------
// The rule moves every row every step; a row's gradient-free steps are replayed when it is next referenced
// (gathered for a forward pass: touch; given a gradient: apply) or when the table is observed (orx_table_sync).
bool orx_adam_rows_lazy(const orx_opt* opt, const orx_table* t) {
    return opt->kind == ORX_ADAM && t->rows < (1LL << 31) && t->owned && getenv("ORX_ADAM_DENSE") == nullptr;
}

// duplicate flags + list of the duplicated rows of `ids` (item role) into the context's dedup buffers
int orx_adam_rows_dedup(orx_ctx* ctx, orx_table* t, const int32_t* ids, int64_t n, ColWindows cw) {
    ENSURE(ctx->d_dflag, ctx->d_dflag_cap, (size_t)n);
    ENSURE(ctx->d_dlist, ctx->d_dlist_cap, (size_t)(n / 2 + 1) * sizeof(uint32_t));
    ENSURE(ctx->d_dcount, ctx->d_dcount_cap, sizeof(int));
    ORX_HIP(hipMemsetAsync(ctx->d_dcount, 0, sizeof(int), ctx->stream));
    DedupArgs d;
    memset(&d, 0, sizeof(d));
    d.uid = ids; d.pid = ids; d.nid = ids; d.id_stride = n;
    d.dflag = ctx->d_dflag; d.dlist = ctx->d_dlist; d.dcount = ctx->d_dcount;
    d.flag_stride = n; d.list_stride = n / 2 + 1;
    d.nU = 0; d.nP = n; d.nN = 0; d.NU = 0; d.NI = t->rows; d.nbu = 0; d.nbi = orx_dedup_buckets(t->rows);
    if (cw.win != nullptr && cw.F > 0 && n % cw.F == 0) { d.col_F = cw.F; d.col_win = cw.win; }
    return orx_launch_dedup(ctx, d, 1);
}

// the table becomes (or stays) lazy under `opt`; every row is current at step `now` when it was not lazy before
static int adam_rows_args(orx_ctx* ctx, orx_opt* opt, orx_table* t, int64_t now, AdamRowsArgs* a) {
    if (t->lazy != nullptr && t->lazy != opt) CHECK(orx_table_sync(t));
    const bool resume = t->lazy == opt;
    OptSlots st;
    CHECK(orx_opt_slots(opt, t, &st));
    memset(a, 0, sizeof(*a));
    CHECK(orx_opt_last(opt, t, !resume, &a->last, now));
    // lr_t entries are uploaded well ahead of use (one small copy per 1024 steps instead of one per step; the kernels
    // fetch them through the scalar cache, so an entry is also in place before any kernel can have cached its line)
    if ((int64_t)opt->lrt_uploaded < opt->t + 2) CHECK(orx_adam_lrt(opt, opt->t + 1024));
    t->lazy = opt;
    a->W = t->w; a->M = st.s0; a->V = st.s1; a->rows = t->rows; a->D = t->dim;
    a->lrt = opt->d_lrt; a->b1 = opt->p0; a->b2 = opt->p1; a->eps = opt->p2;
    a->newton = (1.0f - sqrtf(opt->p1)) <= 1e-3f;
    a->cf = orx_adam_cf_params(opt);
    a->err = ctx->d_err;
    return ORX_OK;
}

int orx_adam_rows_touch(orx_ctx* ctx, orx_opt* opt, orx_table* t, const int32_t* ids, int64_t n, bool have_dedup, ColWindows cw) {
    if (n == 0 || opt->t == 0) return ORX_OK;                // nothing has moved yet
    if (t->lazy != opt) return orx_table_sync(t);           // not lazy under this optimizer: every row is (made) current
    AdamRowsArgs a;
    CHECK(adam_rows_args(ctx, opt, t, opt->t, &a));
    if (!have_dedup) CHECK(orx_adam_rows_dedup(ctx, t, ids, n, cw));
    a.dflag = ctx->d_dflag; a.dlist = (const uint32_t*)ctx->d_dlist; a.dcount = ctx->d_dcount;     // (allocated by the dedup)
    a.ids = ids; a.n = n; a.T = (int)opt->t;
    return orx_launch_adam_rows(ctx, false, a, n / 2 + 1);
}

// step opt->t (the caller has advanced the counter) with per-occurrence gradient rows
int orx_adam_rows_apply(orx_ctx* ctx, orx_opt* opt, orx_table* t, const int32_t* ids, int64_t n, const float* grads, int64_t g_stride,
                        bool have_dedup, ColWindows cw) {
    ORX_ARG(opt->t >= 1, "adam_rows_apply: the step counter has not been advanced");
    CHECK(orx_table_scratch(t));
    AdamRowsArgs a;
    CHECK(adam_rows_args(ctx, opt, t, opt->t - 1, &a));
    if (!have_dedup) CHECK(orx_adam_rows_dedup(ctx, t, ids, n, cw));
    a.dflag = ctx->d_dflag; a.dlist = (const uint32_t*)ctx->d_dlist; a.dcount = ctx->d_dcount;
    a.G = t->gsum; a.ids = ids; a.n = n; a.grads = grads; a.g_stride = g_stride;
    a.T = (int)opt->t; a.lr_T = opt->h_lrt[(size_t)opt->t];
    return orx_launch_adam_rows(ctx, true, a, n / 2 + 1);
}

// the same two operations on a SORTED id list (kernels_rowsort.hip): distinct rows are the heads of the runs, a row's
// gradient rows are summed in position order -- no duplicate flags, no gsum, no atomics.  step: the caller has advanced opt->t.
int orx_adam_rows_sorted(orx_ctx* ctx, orx_opt* opt, orx_table* t, const uint2* sorted, int64_t n, const float* grads, int64_t g_stride, bool step) {
    if (n == 0) return ORX_OK;
    AdamRowsArgs a;
    if (!step) {
        if (opt->t == 0) return ORX_OK;
        if (t->lazy != opt) return orx_table_sync(t);
        CHECK(adam_rows_args(ctx, opt, t, opt->t, &a));
        a.T = (int)opt->t;
        return orx_csr_adam(ctx, false, a, t, sorted, n);
    }
    ORX_ARG(opt->t >= 1, "adam_rows_sorted: the step counter has not been advanced");
    CHECK(adam_rows_args(ctx, opt, t, opt->t - 1, &a));
    a.grads = grads; a.g_stride = g_stride; a.T = (int)opt->t; a.lr_T = opt->h_lrt[(size_t)opt->t];
    return orx_csr_adam(ctx, true, a, t, sorted, n);
}

// TF-2.0 sparse Adam in its literal form (ORX_ADAM_DENSE): summed gradient rows into gsum + a dense-decay sweep of the whole table
int orx_adam_dense_sorted(orx_ctx* ctx, orx_opt* opt, orx_table* t, const uint2* sorted, int64_t n, const float* grads, int64_t g_stride) {
    CHECK(orx_table_scratch(t));
    OptSlots st;
    CHECK(orx_opt_slots(opt, t, &st));
    CHECK(orx_csr_accum(ctx, t, sorted, n, grads, g_stride));
    const double b1 = opt->p0, b2 = opt->p1;
    const double tt = (double)(opt->t > 0 ? opt->t : 1);
    const float lr_t = (float)(opt->lr * std::sqrt(1.0 - std::pow(b2, tt)) / (1.0 - std::pow(b1, tt)));
    return orx_launch_adam_sweep(ctx, t->w, st.s0, st.s1, t->gsum, t->rows * t->dim, lr_t, opt->p0, opt->p1, opt->p2);
}

// rows about to be read by a forward pass: replayed to the lazy optimizer's step (no-op for a table that is current)
int orx_table_touch(orx_table* t, const int32_t* ids, int64_t n) {
    if (t == nullptr || t->lazy == nullptr) return ORX_OK;
    return orx_adam_rows_touch(t->ctx, t->lazy, t, ids, n, false);
}

// Adagrad / momentum on per-occurrence gradient rows: dedup-sum semantics (duplicate flags + gsum + dup_apply)
int orx_summed_rows_apply(orx_ctx* ctx, orx_opt* opt, orx_table* t, orx_table* bias, const int32_t* ids, int64_t n, const float* grads,
                           int64_t g_stride, ColWindows cw) {
    RowsArgs a;
    memset(&a, 0, sizeof(a));
    a.W = t->w; a.bias = bias ? bias->w : nullptr;
    a.ids = ids; a.grads = grads; a.g_stride = g_stride; a.n = n; a.rows = t->rows; a.D = t->dim;
    a.lr = opt->lr; a.err = ctx->d_err;
    CHECK(orx_table_scratch(t));
    if (bias) CHECK(orx_table_scratch(bias));
    OptSlots st, sb;
    CHECK(orx_opt_slots(opt, t, &st));
    if (bias) CHECK(orx_opt_slots(opt, bias, &sb));
    ENSURE(ctx->d_dflag, ctx->d_dflag_cap, (size_t)n);
    ENSURE(ctx->d_dlist, ctx->d_dlist_cap, (size_t)(n / 2 + 1) * sizeof(uint32_t));
    ENSURE(ctx->d_dcount, ctx->d_dcount_cap, sizeof(int));
    ORX_HIP(hipMemsetAsync(ctx->d_dcount, 0, sizeof(int), ctx->stream));
    DedupArgs d;
    memset(&d, 0, sizeof(d));
    // scan the id list in the ITEM role so that dup_apply also finishes the bias
    d.uid = ids; d.pid = ids; d.nid = ids; d.id_stride = n;
    d.dflag = ctx->d_dflag; d.dlist = ctx->d_dlist; d.dcount = ctx->d_dcount;
    d.flag_stride = n; d.list_stride = n / 2 + 1;
    d.nU = 0; d.nP = n; d.nN = 0; d.NU = 0; d.NI = t->rows; d.nbu = 0; d.nbi = orx_dedup_buckets(t->rows);
    if (cw.win != nullptr && cw.F > 0 && n % cw.F == 0) { d.col_F = cw.F; d.col_win = cw.win; }
    CHECK(orx_launch_dedup(ctx, d, 1));
    a.G = t->gsum; a.gb = bias ? bias->gsum : nullptr;
    a.A = st.s0; a.ab = bias ? sb.s0 : nullptr;
    a.dflag = ctx->d_dflag; a.eps = orx_rule_eps(opt);
    CHECK(orx_launch_apply_rows(ctx, opt->kind, true, a));
    PairArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.V = t->w; pa.gV = t->gsum; pa.aV = st.s0;
    pa.b = bias ? bias->w : nullptr; pa.gb = bias ? bias->gsum : nullptr; pa.ab = bias ? sb.s0 : nullptr;
    pa.dlist = ctx->d_dlist; pa.dcount = ctx->d_dcount;
    pa.B = n; pa.D = t->dim; pa.lr = opt->lr; pa.eps = a.eps;
    return orx_launch_dup_apply(ctx, opt->kind, pa);
}

extern "C" int orx_apply_rows(orx_ctx* ctx, orx_opt* opt, orx_table* t, orx_table* bias,
                              const int32_t* ids, int64_t n, const float* grads, int64_t g_stride) {
    const bool lazy = ctx && opt && t && orx_adam_rows_lazy(opt, t);
    if (t && !lazy) CHECK(orx_table_sync(t));
    if (bias && !lazy) CHECK(orx_table_sync(bias));
    ORX_ARG(ctx && opt && t && (n == 0 || (ids && grads)), "orx_apply_rows: NULL argument");
    CHECK(orx_check_apply_rows_opt(opt, t, bias));
    ORX_ARG(g_stride >= t->dim + (bias ? 1 : 0), "orx_apply_rows: g_stride too small");
    ORX_ARG(!bias || (bias->dim == 1 && bias->rows == t->rows), "orx_apply_rows: bias must be [%lld, 1]", (long long)t->rows);
    if (n == 0) return ORX_OK;
    ORX_HIP(hipSetDevice(ctx->device));
    if (bias == nullptr && t->dim <= 256 && getenv("ORX_ROWS_ATOMICS") == nullptr) {
        // the deterministic path (kernels_rowsort.hip): sort the (row, position) pairs, sum every row's gradients in position
        // order, apply the rule once per distinct row
        const uint2* sorted = nullptr;
        CHECK(orx_rows_sort(ctx, ids, 1, n, n, t->rows, &sorted));
        return orx_apply_rows_sorted(ctx, opt, t, sorted, n, grads, g_stride);
    }
    RowsArgs a;
    memset(&a, 0, sizeof(a));
    a.W = t->w; a.bias = bias ? bias->w : nullptr;
    a.ids = ids; a.grads = grads; a.g_stride = g_stride; a.n = n; a.rows = t->rows; a.D = t->dim;
    a.lr = opt->lr; a.err = ctx->d_err;
    if (opt->kind == ORX_SGD) return orx_launch_apply_rows(ctx, ORX_SGD, false, a);
    if (lazy) {             // the bias column is a [rows, 1] table of its own with the same id list (one duplicate analysis)
        CHECK(orx_adam_rows_apply(ctx, opt, t, ids, n, grads, g_stride, false));
        if (bias) CHECK(orx_adam_rows_apply(ctx, opt, bias, ids, n, grads + t->dim, g_stride, true));
        return ORX_OK;
    }
    if (opt->kind == ORX_ADAM) {
        // TF-2.0 sparse Adam: summed gradient rows + a dense-decay sweep of the whole table.
        // The caller advances opt->t once per step (see dlrm.hip).
        CHECK(orx_table_scratch(t));
        OptSlots st;
        CHECK(orx_opt_slots(opt, t, &st));
        CHECK(orx_launch_rows_accum(ctx, t->gsum, ids, grads, g_stride, n, t->dim, t->rows));
        const double b1 = opt->p0, b2 = opt->p1;
        const double tt = (double)(opt->t > 0 ? opt->t : 1);
        const float lr_t = (float)(opt->lr * std::sqrt(1.0 - std::pow(b2, tt)) / (1.0 - std::pow(b1, tt)));
        return orx_launch_adam_sweep(ctx, t->w, st.s0, st.s1, t->gsum, t->rows * t->dim, lr_t, opt->p0, opt->p1, opt->p2);
    }

    return orx_summed_rows_apply(ctx, opt, t, bias, ids, n, grads, g_stride);
}

// ---- planned apply of K id lists against one table (see orx_internal.h) ------------------------------------------
int orx_apply_rows_plan(orx_ctx* c, orx_table* t, const int32_t* ids, int64_t K, int64_t n, int64_t id_stride, RowsPlan* out) {
    out->ready = false;
    if (K == 0 || n == 0) return ORX_OK;
    ORX_ARG(orx_fused_can_inline_apply(t->dim) && t->rows < (1LL << 28), "apply_rows_plan: needs a float4 dim and fewer than 2^28 rows");
    ORX_HIP(hipSetDevice(c->device));
    CHECK(orx_table_scratch(t, true));
    const int nb_total = orx_dedup_buckets(t->rows);
    CHECK(orx_exact_buffers(c, t, t, K, n, MODE_EXACT, true, false, true, nb_total, 1, &out->plan));
    ORX_ARG(out->plan.chunk >= K, "apply_rows_plan: %lld lists of %lld ids exceed one plan chunk (%lld)", (long long)K, (long long)n,
            (long long)out->plan.chunk);
    // the id lists play the ITEM role (so that dup_apply also finishes a bias column); no user list
    CHECK(orx_exact_plan_chunk(c, t, t, ids, ids, ids, id_stride, 0, n, 0, K, n, true, false, true, out->plan, &out->ck));
    out->n = n; out->ready = true;
    return ORX_OK;
}

int orx_apply_rows_planned_step(orx_ctx* c, orx_opt* opt, orx_table* t, orx_table* bias, const RowsPlan& rp, int64_t i,
                                const int32_t* ids, const float* grads, int64_t g_stride) {
    ORX_ARG(opt->kind != ORX_MOMENTUM, "apply_rows_planned_step: momentum is not supported here (the sharded engines are SGD / Adagrad / Adam)");
    ORX_ARG(rp.ready && (opt->kind == ORX_SGD || opt->kind == ORX_ADAGRAD), "apply_rows_planned_step: no plan, or not SGD / Adagrad");
    if (bias) CHECK(orx_table_scratch(bias, true));
    OptSlots st, sb;
    CHECK(orx_opt_slots(opt, t, &st));
    if (bias) CHECK(orx_opt_slots(opt, bias, &sb));
    const int64_t n = rp.n;
    PairArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.V = t->w; pa.gV = t->gsum; pa.gV2 = t->gsum2; pa.aV = st.s0; pa.role_bits = 1;
    pa.b = bias ? bias->w : nullptr; pa.gb = bias ? bias->gsum : nullptr; pa.gb2 = bias ? bias->gsum2 : nullptr; pa.ab = bias ? sb.s0 : nullptr;
    pa.B = n; pa.D = t->dim; pa.lr = opt->lr; pa.eps = opt->kind == ORX_ADAGRAD ? opt->p1 : 0.f;
    orx_exact_step_views(c, rp.plan, i, n, t->dim, rp.ck.use_stage, &pa);
    RowsArgs a;
    memset(&a, 0, sizeof(a));
    a.W = t->w; a.bias = pa.b; a.G = t->gsum; a.G2 = t->gsum2; a.gb = pa.gb; a.gb2 = pa.gb2; a.A = st.s0; a.ab = pa.ab;
    a.ids = ids; a.ids2 = c->d_ids2 + (size_t)i * 3 * rp.plan.Bp + rp.plan.Bp;      // the item list of step i
    a.grads = grads; a.g_stride = g_stride; a.n = n; a.rows = t->rows; a.D = t->dim; a.lr = pa.lr; a.eps = pa.eps; a.err = c->d_err;
    a.refinfo = pa.refinfo ? pa.refinfo + rp.plan.Bp : nullptr; a.segstart = pa.segstart; a.stage = pa.stage; a.stageb = pa.stageb;
    CHECK(orx_launch_rows_planned(c, opt->kind, a));
    for (int l = 0; l < rp.ck.tree_levels; ++l) CHECK(orx_launch_hot_reduce(c, pa, l));
    return orx_launch_dup_apply(c, opt->kind, pa);
}

// duplicate flags of K id lists against a table of `rows` rows: dflag[k*n + i] = 1 iff the row ids[k*id_stride + i]
// occurs more than once in list k (ids < 0 are skipped, their flag is not written)
extern "C" int orx_rows_dupflags(orx_ctx* ctx, int64_t rows, const int32_t* ids, int64_t K, int64_t n, int64_t id_stride,
                                 unsigned char* dflag) {
    ORX_ARG(ctx && rows > 0 && (K == 0 || n == 0 || (ids && dflag)), "orx_rows_dupflags: bad argument");
    if (K == 0 || n == 0) return ORX_OK;
    ORX_HIP(hipSetDevice(ctx->device));
    const int64_t list_stride = n / 2 + 1;
    ENSURE(ctx->d_dlist, ctx->d_dlist_cap, (size_t)K * list_stride * sizeof(uint32_t));
    ENSURE(ctx->d_dcount, ctx->d_dcount_cap, (size_t)K * sizeof(int));
    ORX_HIP(hipMemsetAsync(ctx->d_dcount, 0, (size_t)K * sizeof(int), ctx->stream));
    DedupArgs d;
    memset(&d, 0, sizeof(d));
    d.uid = ids; d.pid = ids; d.nid = ids; d.id_stride = id_stride;
    d.dflag = dflag; d.dlist = ctx->d_dlist; d.dcount = ctx->d_dcount;
    d.flag_stride = n; d.list_stride = list_stride;
    d.nU = 0; d.nP = n; d.nN = 0; d.NU = 0; d.NI = rows; d.nbu = 0; d.nbi = orx_dedup_buckets(rows);
    return orx_launch_dedup(ctx, d, K);
}

// orx_apply_rows for SGD with the duplicate flags of the id list already known (orx_rows_dupflags)
int orx_apply_rows_flagged_impl(orx_ctx* ctx, orx_opt* opt, orx_table* t, orx_table* bias, const int32_t* ids, int64_t n,
                                const float* grads, int64_t g_stride, const float* gbias, const unsigned char* dflag);
extern "C" int orx_apply_rows_flagged(orx_ctx* ctx, orx_opt* opt, orx_table* t, orx_table* bias, const int32_t* ids, int64_t n,
                                      const float* grads, int64_t g_stride, const unsigned char* dflag) {
    return orx_apply_rows_flagged_impl(ctx, opt, t, bias, ids, n, grads, g_stride, nullptr, dflag);
}

static int flagged_args(orx_ctx* ctx, orx_opt* opt, orx_table* t, orx_table* bias, const int32_t* ids, int64_t n,
                        const float* grads, int64_t g_stride, const float* gbias, const unsigned char* dflag, RowsArgs* out) {
    ORX_ARG(!opt || opt->kind != ORX_MOMENTUM, "orx_apply_rows_flagged: SGD only, momentum is not supported (orx_apply_rows takes it)");
    if (t) CHECK(orx_table_sync(t));
    if (bias) CHECK(orx_table_sync(bias));
    ORX_ARG(ctx && opt && t && (n == 0 || (ids && grads && dflag)), "orx_apply_rows_flagged: NULL argument");
    ORX_ARG(opt->kind == ORX_SGD, "orx_apply_rows_flagged: SGD only (Adagrad / Adam: orx_apply_rows)");
    ORX_ARG(g_stride >= t->dim + ((bias && !gbias) ? 1 : 0), "orx_apply_rows_flagged: g_stride too small");
    ORX_ARG(!bias || (bias->dim == 1 && bias->rows == t->rows), "orx_apply_rows_flagged: bias must be [%lld, 1]", (long long)t->rows);
    RowsArgs a;
    memset(&a, 0, sizeof(a));
    a.W = t->w; a.bias = bias ? bias->w : nullptr;
    a.ids = ids; a.grads = grads; a.g_stride = g_stride; a.n = n; a.rows = t->rows; a.D = t->dim;
    a.lr = opt->lr; a.err = ctx->d_err; a.dflag = dflag; a.gbias = gbias;
    *out = a;
    return ORX_OK;
}

// gbias != NULL: the bias gradients come in an array of their own ([n]) instead of column dim of the gradient rows
int orx_apply_rows_flagged_impl(orx_ctx* ctx, orx_opt* opt, orx_table* t, orx_table* bias, const int32_t* ids, int64_t n,
                                const float* grads, int64_t g_stride, const float* gbias, const unsigned char* dflag) {
    RowsArgs a;
    CHECK(flagged_args(ctx, opt, t, bias, ids, n, grads, g_stride, gbias, dflag, &a));
    if (n == 0) return ORX_OK;
    ORX_HIP(hipSetDevice(ctx->device));
    return orx_launch_apply_rows(ctx, ORX_SGD, true, a);
}

int orx_apply_rows_flagged_pair(orx_ctx* ctx, orx_opt* opt, orx_table* tA, orx_table* biasA, const int32_t* idsA, int64_t nA, const float* gA, int64_t strideA,
                                const float* gbiasA, const unsigned char* flagA, orx_table* tB, orx_table* biasB, const int32_t* idsB, int64_t nB, const float* gB,
                                int64_t strideB, const float* gbiasB, const unsigned char* flagB, bool flags_over_both) {
    RowsArgs a, b;
    CHECK(flagged_args(ctx, opt, tA, biasA, idsA, nA, gA, strideA, gbiasA, flagA, &a));
    CHECK(flagged_args(ctx, opt, tB, biasB, idsB, nB, gB, strideB, gbiasB, flagB, &b));
    ORX_HIP(hipSetDevice(ctx->device));
    int rc = ORX_OK;
    // (two lists of ONE table: only where the caller's flags were made over both lists together -- a row in both is then an atomic add in both)
    if ((tA != tB || flags_over_both) && orx_launch_apply_rows_pair(ctx, a, b, &rc)) return rc;
    if (nA) CHECK(orx_launch_apply_rows(ctx, ORX_SGD, true, a));
    if (nB) CHECK(orx_launch_apply_rows(ctx, ORX_SGD, true, b));
    return ORX_OK;
}

// ------------------------------------------------- device-side exchange plan ---
extern "C" int orx_shard_route(orx_ctx* ctx, const int32_t* uid, const int32_t* pid, const int32_t* nid, int64_t B,
                               int64_t users_global, int64_t items_global, int32_t world, int32_t cap,
                               int32_t* send, int32_t* counters, int32_t* overflow) {
    ORX_ARG(ctx && uid && pid && nid && send && counters && overflow, "orx_shard_route: NULL argument");
    ORX_ARG(world >= 1 && world <= 64 && cap >= 1, "orx_shard_route: world must be in [1, 64] and cap positive");
    ORX_HIP(hipSetDevice(ctx->device));
    ORX_HIP(hipMemsetAsync(send, 0xFF, (size_t)world * cap * 3 * sizeof(int32_t), ctx->stream));
    ORX_HIP(hipMemsetAsync(counters, 0, (size_t)world * sizeof(int32_t), ctx->stream));
    RouteArgs a;
    memset(&a, 0, sizeof(a));
    a.uid = uid; a.pid = pid; a.nid = nid; a.B = B; a.world = world; a.cap = cap;
    a.send = send; a.counters = counters; a.overflow = overflow; a.err = ctx->d_err;
    a.NU = users_global; a.NI = items_global;
    return orx_launch_shard_route(ctx, a);
}

// K steps at once (the plan of a K-step call depends on the ids alone): per-step arrays are contiguous,
// uid/pid/nid [K][id_stride], send [K][world*cap][3], counters [K][world]
extern "C" int orx_shard_route_steps(orx_ctx* ctx, const int32_t* uid, const int32_t* pid, const int32_t* nid, int64_t K, int64_t B,
                                     int64_t id_stride, int64_t users_global, int64_t items_global, int32_t world, int32_t cap,
                                     int32_t* send, int32_t* counters, int32_t* overflow) {
    ORX_ARG(ctx && uid && pid && nid && send && counters && overflow, "orx_shard_route_steps: NULL argument");
    ORX_ARG(world >= 1 && world <= 64 && cap >= 1 && K >= 0 && K < 65536, "orx_shard_route_steps: world in [1, 64], cap positive, K < 65536");
    ORX_HIP(hipSetDevice(ctx->device));
    ORX_HIP(hipMemsetAsync(send, 0xFF, (size_t)K * world * cap * 3 * sizeof(int32_t), ctx->stream));
    ORX_HIP(hipMemsetAsync(counters, 0, (size_t)K * world * sizeof(int32_t), ctx->stream));
    RouteArgs a;
    memset(&a, 0, sizeof(a));
    a.uid = uid; a.pid = pid; a.nid = nid; a.B = B; a.world = world; a.cap = cap; a.id_stride = id_stride;
    a.send = send; a.counters = counters; a.overflow = overflow; a.err = ctx->d_err;
    a.NU = users_global; a.NI = items_global;
    return orx_launch_shard_route(ctx, a, K);
}

extern "C" int orx_shard_request_steps(orx_ctx* ctx, const int32_t* trip, int64_t K, int64_t T, int32_t world, int32_t cap,
                                       int32_t* send_ids, int32_t* slot, int32_t* u_loc, int32_t* counters, int32_t* overflow) {
    ORX_ARG(ctx && trip && send_ids && slot && u_loc && counters && overflow, "orx_shard_request_steps: NULL argument");
    ORX_ARG(world >= 1 && world <= 64 && cap >= 1 && K >= 0 && K < 65536, "orx_shard_request_steps: world in [1, 64], cap positive, K < 65536");
    ORX_HIP(hipSetDevice(ctx->device));
    ORX_HIP(hipMemsetAsync(send_ids, 0xFF, (size_t)K * world * cap * sizeof(int32_t), ctx->stream));
    ORX_HIP(hipMemsetAsync(counters, 0, (size_t)K * world * sizeof(int32_t), ctx->stream));
    RequestArgs a;
    memset(&a, 0, sizeof(a));
    a.trip = trip; a.T = T; a.world = world; a.cap = cap;
    a.send_ids = send_ids; a.slot = slot; a.u_loc = u_loc; a.counters = counters; a.overflow = overflow;
    return orx_launch_shard_request(ctx, a, K);
}

// orx_shard_request_steps with per-destination dedup: an item several references of a list ask for claims ONE slot.
// slot[r] of those references is the same, dupref[r] = 1 marks them (their gradients are added into the slot: orx_shard_grads);
// the distinct items of an owner fill its bucket in ascending row order.
extern "C" int orx_shard_request_dedup_steps(orx_ctx* ctx, const int32_t* trip, int64_t K, int64_t T, int32_t world, int32_t cap,
                                             int64_t items_global, int32_t* send_ids, int32_t* slot, int32_t* u_loc,
                                             uint8_t* dupref, void* sorted_out, void* seglist, int32_t* segcount, int32_t* overflow) {
    ORX_ARG(ctx && trip && send_ids && slot && u_loc && dupref && sorted_out && seglist && segcount && overflow, "orx_shard_request_dedup_steps: NULL argument");
    ORX_ARG(world >= 1 && world <= 64 && cap >= 1 && K >= 0 && K < 65536 && items_global > 0, "orx_shard_request_dedup_steps: world in [1, 64], cap positive, K < 65536");
    if (K == 0 || T == 0) return ORX_OK;
    ORX_HIP(hipSetDevice(ctx->device));
    ORX_HIP(hipMemsetAsync(send_ids, 0xFF, (size_t)K * world * cap * sizeof(int32_t), ctx->stream));
    DedupReqArgs a;
    memset(&a, 0, sizeof(a));
    a.trip = trip; a.T = T; a.world = world; a.cap = cap; a.Lr = (items_global + world - 1) / world;
    a.nchunk = (int)((2 * T + 1023) / 1024);
    // scratch: keys [K][2T] | uq [K][2T] | chunkcnt [K][nchunk] | ostart [K][64]
    ENSURE(ctx->d_tmp, ctx->d_tmp_cap, ((size_t)K * 2 * T * 2 + (size_t)K * (a.nchunk + 64)) * sizeof(int32_t));
    a.keys = (int32_t*)ctx->d_tmp; a.uq = a.keys + (size_t)K * 2 * T; a.chunkcnt = a.uq + (size_t)K * 2 * T; a.ostart = a.chunkcnt + (size_t)K * a.nchunk;
    a.send_ids = send_ids; a.slot = slot; a.u_loc = u_loc; a.dupref = dupref; a.overflow = overflow;
    a.seglist = (int2*)seglist; a.segcount = segcount;
    CHECK(orx_launch_shard_keys(ctx, a, K));
    const uint2* sorted = nullptr;
    CHECK(orx_rows_sort(ctx, a.keys, K, 2 * T, 2 * T, (int64_t)world * a.Lr, &sorted));
    // (the context's sort buffers are reused by the next sort -- the applies of the steps sort too: the plan keeps a copy)
    ORX_HIP(hipMemcpyAsync(sorted_out, sorted, (size_t)K * 2 * T * sizeof(uint2), hipMemcpyDeviceToDevice, ctx->stream));
    a.sorted = (const uint2*)sorted_out;
    return orx_launch_shard_dedup_slots(ctx, a, K);
}

extern "C" int orx_shard_request(orx_ctx* ctx, const int32_t* trip, int64_t T, int32_t world, int32_t cap,
                                 int32_t* send_ids, int32_t* slot, int32_t* u_loc, int32_t* counters, int32_t* overflow) {
    ORX_ARG(ctx && trip && send_ids && slot && u_loc && counters && overflow, "orx_shard_request: NULL argument");
    ORX_ARG(world >= 1 && world <= 64 && cap >= 1, "orx_shard_request: world must be in [1, 64] and cap positive");
    ORX_HIP(hipSetDevice(ctx->device));
    ORX_HIP(hipMemsetAsync(send_ids, 0xFF, (size_t)world * cap * sizeof(int32_t), ctx->stream));
    ORX_HIP(hipMemsetAsync(counters, 0, (size_t)world * sizeof(int32_t), ctx->stream));
    RequestArgs a;
    memset(&a, 0, sizeof(a));
    a.trip = trip; a.T = T; a.world = world; a.cap = cap;
    a.send_ids = send_ids; a.slot = slot; a.u_loc = u_loc; a.counters = counters; a.overflow = overflow;
    return orx_launch_shard_request(ctx, a);
}

extern "C" int orx_shard_bucket(orx_ctx* ctx, const int32_t* ids, int64_t n, int32_t world, int32_t cap,
                                int32_t* send_ids, int32_t* slot, int32_t* counters, int32_t* overflow) {
    ORX_ARG(ctx && (n == 0 || ids) && send_ids && slot && counters && overflow, "orx_shard_bucket: NULL argument");
    ORX_ARG(world >= 1 && world <= 64 && cap >= 1, "orx_shard_bucket: world must be in [1, 64] and cap positive");
    ORX_HIP(hipSetDevice(ctx->device));
    ORX_HIP(hipMemsetAsync(send_ids, 0xFF, (size_t)world * cap * sizeof(int32_t), ctx->stream));
    ORX_HIP(hipMemsetAsync(counters, 0, (size_t)world * sizeof(int32_t), ctx->stream));
    return orx_launch_shard_bucket(ctx, ids, n, world, cap, send_ids, slot, counters, overflow);
}

extern "C" int orx_shard_localize(orx_ctx* ctx, const int32_t* ids, int64_t n, int32_t world, int32_t* out) {
    ORX_ARG(ctx && (n == 0 || (ids && out)) && world >= 1, "orx_shard_localize: bad argument");
    ORX_HIP(hipSetDevice(ctx->device));
    return orx_launch_shard_localize(ctx, ids, n, world, out);
}

// Both gradient entry points and the library's own sharded engine.  opt / dup_u / u_apply != NULL: SGD's apply of the user rows
// referenced once folded in.  bias_in / gb_out != NULL: the biases travel apart from the rows (row_stride = D; the side buffer of
// shared slots keeps rows of D + 4 floats with the bias gradient at column D), else at column D of the rows (row_stride > D).
int orx_shard_grads_impl(orx_ctx* ctx, int model, orx_opt* opt, orx_table* user, const float* rows_in, const float* bias_in,
                         const int32_t* u_loc, const int32_t* slot, const uint8_t* dupref, const void* sorted, const void* seglist,
                         const int32_t* segcount, float* gdup, const uint8_t* dup_u, int64_t T, int64_t row_stride, int64_t B_global,
                         float margin, int flags, float* gu, int32_t* u_apply, float* send_g, float* gb_out, double* loss_l2_accum,
                         float* partial_ext, int* nwaves_out) {
    const bool fold = dup_u != nullptr;
    if (fold) CHECK(orx_table_sync(user));
    else if (user && u_loc) CHECK(orx_table_touch(user, u_loc, T));   // a lazy table: the user rows read here are brought up to date
    ORX_ARG(ctx && user && rows_in && u_loc && slot && gu && send_g && (!fold || (opt && u_apply)), "orx_shard_grads: NULL argument");
    ORX_ARG(!fold || opt->kind == ORX_SGD, "orx_shard_grads_sgd: the folded apply is SGD's (Adagrad / Adam sum duplicates first: orx_shard_grads + orx_apply_rows)");
    ORX_ARG(model == ORX_BPR || model == ORX_UCML, "orx_shard_grads: unknown model %d", model);
    ORX_ARG((bias_in != nullptr) == (gb_out != nullptr), "orx_shard_grads: biases in and bias gradients out travel apart together");
    ORX_ARG((bias_in ? row_stride >= user->dim : row_stride > user->dim) && B_global > 0, "orx_shard_grads: row_stride must leave room for the bias column");
    ORX_ARG(!dupref || (sorted && seglist && segcount && gdup), "orx_shard_grads: dedup needs the plan's sorted list, segment list and a side buffer");
    if (T == 0) return ORX_OK;
    ORX_HIP(hipSetDevice(ctx->device));
    ShardGradArgs a;
    memset(&a, 0, sizeof(a));
    a.U = user->w; a.rows_in = rows_in; a.u_loc = u_loc; a.slot = slot; a.gu = gu; a.send_g = send_g; a.dupref = dupref; a.gdup = gdup;
    a.bias_in = bias_in; a.gb_out = gb_out;
    a.T = T; a.D = user->dim; a.DS = (int)row_stride; a.DSg = bias_in ? user->dim + 4 : (int)row_stride;
    a.invB = 1.0f / (float)B_global; a.margin = margin; a.l2w = (flags & ORX_NO_L2) ? 0.f : 1.f;
    if (fold) { a.fu = dup_u; a.Uw = user->w; a.lr = opt->lr; a.u_apply = u_apply; }
    // partial_ext (the library's engine): the launch's loss partials stay in the caller's buffer, which adds a whole chunk of steps
    // to the sums with ONE launch (a launch per step and half cost 4 us + a kernel boundary of every 84 us step)
    if (partial_ext == nullptr) ENSURE(ctx->d_partial, ctx->d_partial_cap, (size_t)(T + 4) * 2 * sizeof(float));
    a.partial = partial_ext ? partial_ext : ctx->d_partial;
    int nw = 0;
    CHECK(orx_launch_shard_grads(ctx, model, a, &nw));
    if (nwaves_out) *nwaves_out = nw;
    if (dupref) CHECK(orx_launch_shard_segsum(ctx, (const int2*)seglist, segcount, (const uint2*)sorted, 2 * T, gdup, a.DSg, send_g, a.DS, a.D, gb_out));
    if (loss_l2_accum && partial_ext == nullptr) CHECK(orx_launch_loss_accumulate(ctx, ctx->d_partial, nw, loss_l2_accum));
    return ORX_OK;
}

extern "C" int orx_shard_grads(orx_ctx* ctx, int model, orx_table* user, const float* rows_in, const int32_t* u_loc,
                               const int32_t* slot, const uint8_t* dupref, const void* sorted, const void* seglist, const int32_t* segcount,
                               float* gdup, int64_t T, int64_t row_stride, int64_t B_global, float margin, int flags,
                               float* gu, float* send_g, double* loss_l2_accum) {
    return orx_shard_grads_impl(ctx, model, nullptr, user, rows_in, nullptr, u_loc, slot, dupref, sorted, seglist, segcount, gdup, nullptr, T, row_stride,
                                B_global, margin, flags, gu, nullptr, send_g, nullptr, loss_l2_accum);
}

// orx_shard_grads with the SGD apply of the (local) user rows folded in: rows referenced once in the step are updated in
// place by the gradient kernel, the references of duplicated rows leave (u_apply[t] = local row, gu[t] = gradient) for
// orx_apply_rows_flagged; u_apply[t] = -1 everywhere else.  dup_u: the flags orx_rows_dupflags made for u_loc.
extern "C" int orx_shard_grads_sgd(orx_ctx* ctx, int model, orx_opt* opt, orx_table* user, const float* rows_in, const int32_t* u_loc,
                                   const int32_t* slot, const uint8_t* dupref, const void* sorted, const void* seglist, const int32_t* segcount,
                                   float* gdup, const uint8_t* dup_u, int64_t T, int64_t row_stride, int64_t B_global,
                                   float margin, int flags, float* gu, int32_t* u_apply, float* send_g, double* loss_l2_accum) {
    ORX_ARG(!opt || opt->kind != ORX_MOMENTUM, "orx_shard_grads_sgd: momentum is not supported by the sharded engines");
    ORX_ARG(opt && dup_u && u_apply, "orx_shard_grads_sgd: NULL argument");
    return orx_shard_grads_impl(ctx, model, opt, user, rows_in, nullptr, u_loc, slot, dupref, sorted, seglist, segcount, gdup, dup_u, T, row_stride,
                                B_global, margin, flags, gu, u_apply, send_g, nullptr, loss_l2_accum);
}
