// The host driver of the exact train steps: the BPR / UCML step (orx_pairwise_step*) and the GMF / WRMF step
// (orx_pointwise_step*) with their forward-only calls and orx_pairwise_reserve.  One function decides a call's form, one prepares
// tables, optimizer and buffers, one fills the PairArgs view of the tables, one sets a step's arguments and one runs a chunk of
// steps; a family supplies its traits (ExactTraits), its fused launch and the few passes only it has.  Host code only: the plan's
// host side is in api.hip, the kernels in kernels_{plan,pairwise,pointwise}.hip.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>

#include "orx_internal.h"

// ---- host setup that the pairwise and the pointwise step call share
// ORX_FORCE_FALLBACK (debug / tests; read per call): bit 0 = behave as if the tables had >= 2^28 rows (no role bits: every
// duplicate uses atomics, separate dup_apply launches), bit 1 = no in-launch apply, bit 2 = the censor in separate passes,
// bit 3 = atomics instead of staging slots, bit 4 = no pairing
int orx_fallback_bits() {
    const char* e = getenv("ORX_FORCE_FALLBACK");
    return e ? atoi(e) : 0;
}

// epochs are consumed one per step; on wrap-around every table clears its epoch-tagged arrays
int orx_epochs_reserve(orx_ctx* c, int64_t K, std::initializer_list<orx_table*> tables) {
    if ((int64_t)c->epoch + K + 16 > 0x7fffffff) { c->epoch = 0; c->epoch_gen += 1; }
    for (orx_table* t : tables) {
        if (t->tag_gen != c->epoch_gen) {
            if (t->ready) ORX_HIP(hipMemsetAsync(t->ready, 0, (size_t)t->rows * sizeof(int), c->stream));
            if (t->side) ORX_HIP(hipMemsetAsync(t->side, 0, (size_t)t->rows * 2 * sizeof(int), c->stream));
            t->tag_gen = c->epoch_gen;
        }
    }
    return ORX_OK;
}

// blocks of a step's launch that apply the duplicated rows of the step before it: one lane group per duplicated row in a single
// pass for the usual ~0.15*B duplicated rows (the count lives in device memory; surplus blocks exit, a larger count grid-strides)
int orx_apply_blocks(int64_t B, int D) {
    return (int)std::min<int64_t>(2048, std::max<int64_t>(16, (B / 4) / (1024 / D) + 1));
}

// one step of the dense TF-2.0 Adam (MODE_ACCUM): the counter advances, then the decay sweep over every table whole (NULL: skipped)
int orx_adam_dense_step(orx_ctx* c, orx_opt* opt, std::initializer_list<std::pair<orx_table*, OptSlots>> tables, float* lr_t_out) {
    opt->t += 1;
    const double b1 = opt->p0, b2 = opt->p1;
    const float lr_t = (float)(opt->lr * std::sqrt(1.0 - std::pow(b2, (double)opt->t)) / (1.0 - std::pow(b1, (double)opt->t)));
    for (const auto& ts : tables) {
        orx_table* t = ts.first;
        if (t) CHECK(orx_launch_adam_sweep(c, t->w, ts.second.s0, ts.second.s1, t->gsum, t->rows * t->dim, lr_t, opt->p0, opt->p1, opt->p2));
    }
    if (lr_t_out) *lr_t_out = lr_t;
    return ORX_OK;
}

// ---- the driver
// Where the two families part in the decisions below (DESIGN 4.5za lists which of these the kernels need and which are history).
struct ExactTraits {
    bool lazy_needs_roles;          // lazy Adam is off under fallback bit 0
    bool roles_need_fast_dim;       // role bits on the float4 dims only
    bool byte_flags;                // exact mode without role bits: the family's own byte-flag plan (ExactCall::flags), not the shared one
    bool inline_needs_v2;           // the in-launch apply only beside the bucketed plan
    bool scratch_in_hogwild;        // scratch rows also for a hogwild call
    bool no_readback;               // a call whose predecessor was quiet plans without the host wait (plan_stats_poll, api.hip)
    bool early_launch;              // a chunk's first fused launch goes out before the host waits for the plan's counters
    bool tail_launch;               // the last step's duplicate apply and the chunk's loss sums in one launch
    const char* no_pair_env;        // a switch of its own that turns pairing off (NULL: none)
};
static const ExactTraits PAIR_TRAITS = {false, false, false, false, false, true, true, true, nullptr};
static const ExactTraits POINT_TRAITS = {true, true, true, true, true, false, false, false, "ORX_POINT_NO_PAIR"};

// The form an exact call takes, from the optimizer, the tables, the call's flags and the fallback bits alone: the step runs it,
// orx_pairwise_reserve (flags 0, no fallback bits) sizes the buffers for it.
struct ExactForm {
    bool lazy_adam;
    int mode;
    bool role_bits, fused_censor, censor, inline_apply, staging;
    bool plan;                  // exact mode through the shared plan (orx_exact_plan_chunk): ids rewritten, duplicate lists
};
static ExactForm exact_form(const ExactTraits& tr, const orx_opt* opt, const orx_table* U, const orx_table* V, const orx_table* b, int64_t K,
                            int flags, int fb) {
    ExactForm f;
    const bool hogwild = (flags & ORX_HOGWILD) != 0, want_censor = (flags & ORX_CENSOR) != 0;
    const bool fast_dim = orx_fused_can_inline_apply(U->dim) != 0, small_tables = U->rows < (1LL << 28) && V->rows < (1LL << 28);
    // TF-2.0 Adam decays m, v and moves var on EVERY row every step.  On the float4 dims that is applied lazily and
    // exactly: a row's gradient-free steps are replayed when the row is next touched (or observed: orx_table_sync);
    // the dense form (every reference accumulates, then three whole-table sweeps per step) remains for the other
    // cases and behind ORX_ADAM_DENSE=1.  (Wrapped memory is read behind our back: never lazy.)
    f.lazy_adam = opt->kind == ORX_ADAM && !hogwild && fast_dim && small_tables && !(tr.lazy_needs_roles && (fb & 1)) &&
                  U->owned && V->owned && (!b || b->owned) && getenv("ORX_ADAM_DENSE") == nullptr;
    f.mode = (opt->kind == ORX_ADAM && !f.lazy_adam) ? MODE_ACCUM : (hogwild ? MODE_HOGWILD : MODE_EXACT);
    // rows referenced exactly twice get plain stores into two scratch rows; the role of a reference
    // travels in bits 30:29 of its id, which needs tables below 2^29 rows
    f.role_bits = f.mode == MODE_EXACT && small_tables && (fast_dim || !tr.roles_need_fast_dim) && !(fb & 1);
    f.plan = f.mode == MODE_EXACT && (f.role_bits || !tr.byte_flags);
    // censor_vec after every step (ucml.py:44-48): fused into the row write-back for the float4 dims in
    // exact mode; separate passes otherwise
    f.fused_censor = want_censor && f.mode == MODE_EXACT && fast_dim && !(fb & 4);
    f.censor = want_censor && !f.fused_censor;
    // the previous step's duplicated rows are applied by extra blocks of the next step's launch
    // (no dup_apply launch, no kernel boundary) -- not with a separate censor pass between the steps
    f.inline_apply = f.role_bits && !f.censor && K > 1 && fast_dim && (!tr.inline_needs_v2 || orx_plan_v2(true)) && !(fb & 2);
    // rows referenced >= 3 times in a step: private staging slots instead of atomics
    f.staging = f.role_bits && fast_dim && !(fb & 8);
    return f;
}

// one exact call on its way from its entry point through exact_prepare and exact_view to exact_run
struct ExactCall {
    orx_ctx* c; orx_opt* opt; orx_table* U; orx_table* V; orx_table* b;      // b NULL: BPR without item biases
    int64_t K, B;
    const int32_t* ids[3]; int64_t nN; int64_t ds;      // the id lists on the device (pointwise: two, nN = 0, ids[2] = ids[1]), elements between steps
    const float* label = nullptr;       // pointwise: the labels, which ride in the pairing records (c->plan_label)
    bool want_loss;
    int np;                     // (loss, l2) partial slots per step
    ExactForm f;
    bool lazy_resume;           // lazy Adam: the tables were lazy under this optimizer already (their step stamps hold)
    bool nowait = false;        // no read-back (see plan_stats_poll): the previous call of this shape was quiet
    int64_t stats_key[5];
    OptSlots sU, sV, sb;
    PairPlan plan;
    PairArgs a;                 // the one view of the tables: the pairwise kernels' arguments, and what dup_apply / hot_reduce / the in-launch apply of either family read
    float lr_t = 0.f;           // dense Adam: lr_t of the step just swept
    // what the family supplies
    std::function<int(int64_t, int64_t)> launch;        // the fused launch of step s = chunk step i, `a` set for it
    std::function<int(int64_t, int64_t)> flags;         // byte-flag passes of its own over steps s0 .. s0 + kc - 1, after the shared plan (empty: none)
    std::function<int(int64_t, int64_t, int64_t)> after_step;      // what follows the applies of step s0 + i of kc (empty: nothing)
};

// every buffer of a call of this form: scratch rows, optimizer slots, the plan's arrays, the pairing records
static int exact_reserve(ExactCall& q, const ExactTraits& tr, bool pairing) {
    orx_table *U = q.U, *V = q.V, *b = q.b;
    const ExactForm& f = q.f;
    if (f.mode != MODE_HOGWILD || tr.scratch_in_hogwild) {
        CHECK(orx_table_scratch(U, f.role_bits)); CHECK(orx_table_scratch(V, f.role_bits));
        if (b) CHECK(orx_table_scratch(b, f.role_bits));
    }
    CHECK(orx_opt_slots(q.opt, U, &q.sU)); CHECK(orx_opt_slots(q.opt, V, &q.sV));
    if (b) CHECK(orx_opt_slots(q.opt, b, &q.sb));
    const int nb_total = orx_dedup_buckets(U->rows) + orx_dedup_buckets(V->rows);
    // (a family with byte flags of its own sizes them itself: none of the plan's arrays then)
    CHECK(orx_exact_buffers(q.c, U, V, q.K, q.B, f.mode == MODE_EXACT && !f.plan ? MODE_HOGWILD : f.mode, f.role_bits, f.inline_apply, f.staging,
                            nb_total, q.np, &q.plan));
    if (pairing) CHECK(orx_pairing_buffers(q.c, q.B, U->dim, &q.plan));
    return ORX_OK;
}

// tables and optimizer brought to the call's form, the read-back decision, every buffer of the call
static int exact_prepare(ExactCall& q, const ExactTraits& tr, int kmodel, bool weighted, int fb) {
    orx_ctx* c = q.c; orx_opt* opt = q.opt; orx_table *U = q.U, *V = q.V, *b = q.b;
    ExactForm& f = q.f;
    // the three tables are lazy together under one optimizer (the item rows and their biases then share step stamps),
    // or not at all: anything else first brings every row up to date
    q.lazy_resume = f.lazy_adam && U->lazy == opt && V->lazy == opt && (!b || b->lazy == opt);
    if (!q.lazy_resume) for (orx_table* t : {U, V, b}) CHECK(orx_table_sync(t));      // (NULL: nothing to do)
    { orx_table* mine[3] = {U, V, b}; CHECK(orx_opt_isolate(opt, mine, b ? 3 : 2)); }      // (a shared optimizer: see orx_opt_isolate)
    if (tr.no_readback) {
        // (kmodel: a biased and a bias-free call of one shape run different kernels and keep apart; so do a weighted and an unweighted call)
        const bool want_censor = f.censor || f.fused_censor;
        const int64_t key[5] = {q.B, U->rows, V->rows, (int64_t)kmodel * 16 + opt->kind + (weighted ? 1024 : 0), (int64_t)U->dim * 4 + (want_censor ? 1 : 0) + (f.inline_apply ? 2 : 0)};
        CHECK(plan_stats_poll(c));
        const bool plan_wait = getenv("ORX_PLAN_WAIT") != nullptr;      // (experiments / tests: always read back)
        q.nowait = f.mode == MODE_EXACT && orx_plan_v2(f.role_bits) && f.staging && !f.censor && opt->kind != ORX_ADAM && !plan_wait &&
                   c->plan_stats.valid && c->plan_stats.quiet;
        for (int k = 0; k < 5; ++k) { q.stats_key[k] = key[k]; q.nowait = q.nowait && c->plan_stats.key[k] == key[k]; }
        if (q.nowait) f.staging = false;
    }
    // pairing (kernels_plan.hip): the two triplets of a row referenced exactly twice share a wavefront and exchange gradients there
    // (SGD only -- Adagrad with pairing measured slower, profiles/r5_adagrad_pairing_ab.txt -- on the float4 dims with >= 2 triplets per wavefront; fb bit 4 / ORX_NO_PAIR=1: off)
    // The pairing plan costs ~1.5 us per step (records, decisions, the swaps); it pays where a good share of the batch pairs
    // (uniform ids over tables ~ 10 x the batch: 11 %).  Tables so small that most duplicated rows have three or more references, or
    // ids so skewed that the hot rows take them, pair little: the plan of a call tells (accepted pairs per step), and pairing then
    // pauses for 32 calls before it is tried again.  ORX_PAIR_ALWAYS=1: no pause.
    bool pairing = orx_pairing_wanted(f.mode, f.role_bits, opt->kind, U->dim, q.B, fb) && (!tr.no_pair_env || getenv(tr.no_pair_env) == nullptr);
    if (pairing && c->pair_pause > 0) { c->pair_pause -= 1; pairing = false; }
    CHECK(exact_reserve(q, tr, pairing));
    // Adam's normalised update amplifies summation-order noise where an element's summed gradient nearly cancels: its
    // rows referenced >= 3 times always take staging slots (fixed summation order), never fp32 atomics
    if (opt->kind == ORX_ADAM) q.plan.min_late = 1;
    return ORX_OK;
}

// the view's fields that hold for every step of the call (the family adds its own: margin, weights, censor marks ...)
static int exact_view(ExactCall& q) {
    orx_ctx* c = q.c; orx_opt* opt = q.opt; orx_table *U = q.U, *V = q.V, *b = q.b;
    const ExactForm& f = q.f;
    PairArgs& a = q.a;
    memset(&a, 0, sizeof(a));
    a.U = U->w; a.V = V->w; a.b = b ? b->w : nullptr;
    a.gU = U->gsum; a.gV = V->gsum; a.gb = b ? b->gsum : nullptr;
    if (f.role_bits) { a.gU2 = U->gsum2; a.gV2 = V->gsum2; a.gb2 = b ? b->gsum2 : nullptr; a.role_bits = 1; a.readyU = U->ready; a.readyV = V->ready; }
    a.aU = q.sU.s0; a.aV = q.sV.s0; a.ab = q.sb.s0;
    a.B = q.B; a.NU = U->rows; a.NI = V->rows; a.D = U->dim;
    a.lr = opt->lr;
    a.eps = orx_rule_eps(opt);
    a.invB = 1.0f / (float)q.B;
    a.err = c->d_err;
    if (f.lazy_adam) CHECK(orx_lazy_adam_fill(opt, U, V, b, q.sU, q.sV, q.sb, !q.lazy_resume, q.K, &a));
    return orx_epochs_reserve(c, q.K, {U, V});
}

// the view of step i of the chunk that starts at step s0 (with_apply: its launch also applies the duplicated rows of step i - 1);
// the one place where a step takes its epoch and lazy Adam its step
static void exact_step(ExactCall& q, int64_t s0, int64_t i, bool stage_views, bool with_apply) {
    orx_ctx* c = q.c;
    PairArgs& a = q.a;
    const PairPlan& plan = q.plan;
    const int64_t s = s0 + i, B = q.B;
    if (q.f.plan) {         // ids rewritten by the plan (duplicate flag in bit 31)
        a.uid = c->d_ids2 + (size_t)i * 3 * plan.Bp; a.pid = a.uid + plan.Bp; a.nid = a.uid + 2 * plan.Bp;
    } else {
        a.uid = q.ids[0] + s * q.ds; a.pid = q.ids[1] + s * q.ds; a.nid = q.ids[2] + s * q.ds;
    }
    orx_exact_step_views(c, plan, i, B, a.D, stage_views, &a);
    if (!q.b) { a.stageb = nullptr; a.partb = nullptr; a.prev_stageb = nullptr; }      // (no bias: nothing is staged for it)
    a.ids4 = plan.pair_tpw > 1 ? c->d_ids4 + (size_t)i * B : nullptr;
    a.partial = c->d_partial + (size_t)i * q.np * 2;
    a.epoch = ++c->epoch;           // one epoch per step: ready flags and censor side marks are tagged with it
    if (q.f.lazy_adam) { q.opt->t += 1; a.step_t = (int)q.opt->t; }
    if (with_apply && i > 0) {
        a.n_apply_blocks = orx_apply_blocks(B, a.D);
        a.prev_dlist = c->d_dlist + (size_t)(i - 1) * plan.list_stride; a.prev_dcount = c->d_dcount + (i - 1);
    } else {
        a.n_apply_blocks = 0; a.prev_dlist = nullptr; a.prev_dcount = nullptr;
    }
}

// steps s0 .. s0 + kc - 1: their plan, their launches, their loss sums
static int exact_run_chunk(ExactCall& q, const ExactTraits& tr, int64_t s0, int64_t kc) {
    orx_ctx* c = q.c; orx_opt* opt = q.opt; orx_table *U = q.U, *V = q.V, *b = q.b;
    const ExactForm& f = q.f;
    PairArgs& a = q.a;
    const int64_t B = q.B, ds = q.ds;
    const int32_t *du = q.ids[0] + s0 * ds, *dp = q.ids[1] + s0 * ds, *dn = q.ids[2] + s0 * ds;      // step 0 of the chunk
    const bool v2 = f.plan && orx_plan_v2(f.role_bits);
    bool first_launched = false;
    bool tail_done = false;             // the chunk's loss sums left with the last step's duplicate apply
    ExactChunk ck;                      // (no read-back: in-launch apply where the call allows it, no staging, no tree)
    if (q.nowait) {
        CHECK(orx_exact_plan_issue(c, U, V, du, dp, dn, ds, B, B, q.nN, kc, B, f.inline_apply, f.staging, q.plan, 0, nullptr, nullptr));
        ht_mark("plan_issued");
    } else if (f.plan) {
        // With the bucketed plan the chunk's FIRST fused launch goes out before the host waits for the plan's counters:
        // step 0 never carries apply blocks, and the kernel built with the staging bookkeeping is right whether or not
        // any range made a staging plan (references without one carry (-1, 0) and use atomics).
        const std::function<int()> early = [&]() -> int { first_launched = true; exact_step(q, s0, 0, f.staging, false); return q.launch(s0, 0); };
        c->plan_label = q.plan.pair_tpw > 1 && q.label ? q.label + s0 * ds : nullptr;
        const int rc_plan = orx_exact_plan_chunk(c, U, V, du, dp, dn, ds, B, B, q.nN, kc, B, f.role_bits, f.inline_apply, f.staging, q.plan, &ck,
                                                 tr.early_launch && v2 && !f.censor ? &early : nullptr);
        c->plan_label = nullptr;
        CHECK(rc_plan);
    }
    if (q.flags) CHECK(q.flags(s0, kc));
    const ReduceArgs r = {c->d_partial, c->d_loss + 2 * s0, q.np};
    // may the duplicated rows of a step be applied by the NEXT step's launch?  (many duplicated rows / reduction-tree levels: separate launches)
    const bool inl = f.inline_apply && !ck.hot && !ck.dense_dups;
    for (int64_t i = 0; i < kc; ++i) {
        const bool defer = inl && i < kc - 1;      // step i's duplicated rows wait for launch i + 1
        if (!(i == 0 && first_launched)) { exact_step(q, s0, i, ck.use_stage, i > 0 && inl); CHECK(q.launch(s0 + i, i)); }
        for (int l = 0; l < ck.tree_levels; ++l) CHECK(orx_launch_hot_reduce(c, a, l));
        if (f.mode == MODE_EXACT && !defer) {
            // the chunk's last step: its duplicated rows and the chunk's loss sums leave in ONE launch where that is possible
            if (tr.tail_launch && i == kc - 1 && !f.censor && !f.lazy_adam && q.want_loss) {
                int rc = ORX_OK;
                if (orx_launch_tail(c, opt->kind, a, r, kc, &rc)) { CHECK(rc); tail_done = true; }
            }
            if (!tail_done) CHECK(orx_launch_dup_apply(c, opt->kind, a));
        }
        // Adam, dense form: the decay sweep of TF 2.0 over the whole tables
        if (f.mode == MODE_ACCUM) CHECK(orx_adam_dense_step(c, opt, {{U, q.sU}, {V, q.sV}, {b, q.sb}}, &q.lr_t));
        if (q.after_step) CHECK(q.after_step(s0, i, kc));
    }
    if (!tail_done && q.want_loss) CHECK(orx_launch_loss_reduce(c, r, kc));
    if (v2 && tr.no_readback) {
        // what this chunk's plan counted: left behind the last launch for the next call (no read-back), or seen already
        if (q.nowait) CHECK(plan_stats_leave(c, kc, B, q.plan.pair_tpw > 1, q.stats_key));
        else {
            c->plan_stats.valid = true; c->plan_stats.quiet = ck.quiet; c->stats_pending = false;
            for (int k = 0; k < 5; ++k) c->plan_stats.key[k] = q.stats_key[k];
        }
    }
    return ORX_OK;
}

// the chunk loop of a prepared call, its losses and, for host ids, the index flag
static int exact_run(ExactCall& q, const ExactTraits& tr, int flags, float* loss_out, float* l2_out) {
    ht_mark("setup");
    for (int64_t s0 = 0; s0 < q.K; s0 += q.plan.chunk) CHECK(exact_run_chunk(q, tr, s0, std::min<int64_t>(q.K - s0, q.plan.chunk)));
    ht_mark("launched");
    CHECK(fetch_losses(q.c, q.K, loss_out, l2_out));
    ht_mark("losses"); ht_dump();
    if (!(flags & ORX_IDS_DEVICE)) return orx_check_index_error(q.c);
    return ORX_OK;
}

// ------------------------------------------------------------ pairwise (BPR / UCML) ---
// b == NULL: BPR without item biases (model < 0: any model may go without, as in orx_pairwise_reserve); UCML and the
// censor always need the bias
static int check_pair_tables(orx_table* U, orx_table* V, orx_table* b, int model = -1, int flags = 0) {
    ORX_ARG(U && V, "pairwise: NULL table");
    ORX_ARG(b || model != ORX_UCML, "pairwise: UCML needs the item bias table (bias may be NULL with ORX_BPR only)");
    ORX_ARG(b || !(flags & ORX_CENSOR), "pairwise: ORX_CENSOR needs the item bias table (bias may be NULL with ORX_BPR only)");
    if (b == nullptr) {
        ORX_ARG(U->ctx == V->ctx, "pairwise: tables belong to different contexts");
        ORX_ARG(U->dim == V->dim, "pairwise: user dim %d != item dim %d (every model multiplies them element-wise)", U->dim, V->dim);
        return ORX_OK;
    }
    ORX_ARG(U->ctx == V->ctx && V->ctx == b->ctx, "pairwise: tables belong to different contexts");
    ORX_ARG(U->dim == V->dim, "pairwise: user dim %d != item dim %d (every model multiplies them element-wise)", U->dim, V->dim);
    ORX_ARG(b->dim == 1 && b->rows == V->rows, "pairwise: item_bias must be [%lld, 1]", (long long)V->rows);
    return ORX_OK;
}

extern "C" int orx_pairwise_step(orx_ctx* c, int model, orx_opt* opt,
                                 orx_table* U, orx_table* V, orx_table* b,
                                 const int32_t* uid, const int32_t* pid, const int32_t* nid,
                                 int64_t K, int64_t B, int64_t id_stride, float margin, int flags,
                                 float* loss_out, float* l2_out) {
    return orx_pairwise_step_impl(c, model, opt, U, V, b, uid, pid, nid, nullptr, K, B, id_stride, margin, (flags & ORX_NO_L2) ? 0.f : 1.f, flags,
                                  loss_out, l2_out);
}

struct PairStep { ExactCall q; int kmodel; const float* dw; };      // dw: per-triplet weights on the device (NULL: none)

// the censor in separate passes (UCML on the generic dims, dense Adam, fallback bit 2): one elected reference per distinct row of
// each of the three id lists for every step of the chunk, then ucml.py:44-48 after each step
static int pair_censor_flags(ExactCall& q, int64_t s0, int64_t kc) {
    orx_ctx* c = q.c;
    ENSURE(c->d_cflag, c->d_cflag_cap, (size_t)3 * kc * q.B);
    const int64_t rows[3] = {q.U->rows, q.V->rows, q.V->rows};
    for (int l = 0; l < 3; ++l) {
        DedupArgs d;
        memset(&d, 0, sizeof(d));
        d.uid = d.pid = d.nid = q.ids[l] + s0 * q.ds; d.id_stride = q.ds;
        d.dflag = c->d_cflag + (size_t)l * kc * q.B; d.flag_stride = q.B;
        d.nU = q.B; d.NU = rows[l]; d.nbu = orx_dedup_buckets(rows[l]); d.first_only = 1;
        CHECK(orx_launch_dedup(c, d, kc));
    }
    return ORX_OK;
}
static int pair_censor_step(ExactCall& q, int64_t s0, int64_t i, int64_t kc) {      // users and pos items (two tables), then neg items
    orx_ctx* c = q.c; orx_table *U = q.U, *V = q.V;
    const int64_t B = q.B, at = (s0 + i) * q.ds;
    const unsigned char* fu = c->d_cflag + (size_t)i * B;
    const unsigned char* fp = c->d_cflag + (size_t)(kc + i) * B;
    const unsigned char* fn = c->d_cflag + (size_t)(2 * kc + i) * B;
    CHECK(orx_launch_censor2(c, U->w, fu, U->rows, q.ids[0] + at, B, V->w, fp, V->rows, q.ids[1] + at, B, U->dim, 0.1f));
    return orx_launch_censor2(c, V->w, fn, V->rows, q.ids[2] + at, B, nullptr, nullptr, 0, nullptr, 0, U->dim, 0.1f);
}

// The full pairwise step behind orx_pairwise_step (weight NULL, l2w 0 or 1) and orx_pairwise_step_weighted: `weight` lives where the
// ids live and has their stride; l2w is the coefficient of l2_loss in the objective.  A weighted call runs the WT instantiations of the fused
// kernels (kernels_pairwise_weighted.hip) and keeps plan statistics of its own.
int orx_pairwise_step_impl(orx_ctx* c, int model, orx_opt* opt, orx_table* U, orx_table* V, orx_table* b,
                           const int32_t* uid, const int32_t* pid, const int32_t* nid, const float* weight,
                           int64_t K, int64_t B, int64_t id_stride, float margin, float l2w, int flags,
                           float* loss_out, float* l2_out) {
    ORX_ARG(c && opt, "orx_pairwise_step: NULL context/optimizer");
    ORX_ARG(model == ORX_BPR || model == ORX_UCML, "orx_pairwise_step: unknown model %d", model);
    CHECK(check_pair_tables(U, V, b, model, flags));
    ORX_ARG(U->ctx == c && opt->ctx == c, "orx_pairwise_step: objects belong to a different context");
    ORX_ARG(K >= 0 && B >= 0, "orx_pairwise_step: negative K or B");
    ORX_ARG(K == 0 || B == 0 || (uid && pid && nid), "orx_pairwise_step: NULL id pointer");
    if (K == 0) return ORX_OK;
    ht_mark("enter", true);
    ORX_HIP(hipSetDevice(c->device));
    if (B == 0) {           // empty batch: reduce_mean of nothing is NaN in TF; tables untouched
        for (int64_t s = 0; s < K; ++s) { if (loss_out) loss_out[s] = model == ORX_BPR ? NAN : 0.f; if (l2_out) l2_out[s] = 0.f; }
        return ORX_OK;
    }
    PairStep p;
    ExactCall& q = p.q;
    q.c = c; q.opt = opt; q.U = U; q.V = V; q.b = b; q.K = K; q.B = B;
    p.kmodel = b ? model : MODEL_BPR_NB;        // b == NULL: the kernels of MODEL_BPR_NB, every use of the bias table is skipped
    q.want_loss = loss_out != nullptr || l2_out != nullptr;
    q.np = orx_fused_nwaves(U->dim, B);
    StepInputs in;
    CHECK(orx_stage_steps(c, K, B, id_stride, flags, {{uid, 1}, {pid, 1}, {nid, 1}}, {{weight, 1}}, &in));
    q.ids[0] = in.id[0]; q.ids[1] = in.id[1]; q.ids[2] = in.id[2]; q.nN = B; p.dw = in.f[0]; q.ds = in.ds;
    ORX_ARG(!(flags & ORX_HOGWILD) || opt->kind != ORX_MOMENTUM, "orx_pairwise_step: ORX_HOGWILD is not supported with momentum (its racy in-place pass has no velocity rule)");
    const int fb = orx_fallback_bits();
    q.f = exact_form(PAIR_TRAITS, opt, U, V, b, K, flags, fb);
    CHECK(exact_prepare(q, PAIR_TRAITS, p.kmodel, p.dw != nullptr, fb));
    CHECK(exact_view(q));
    PairArgs& a = q.a;
    a.margin = margin;
    a.l2w = l2w;
    // Neither the loss nor the l2 sum is asked for (a training loop between two observations of the loss): the kernels that have a
    // loss-free form (fused_kernel LOSS = false: exact SGD on the float4 dims, unweighted) skip their partials, and for every kernel
    // the sums over the partials are not launched -- d_partial and d_loss are read by nothing but the fetch_losses of the call itself
    a.no_loss = q.want_loss ? 0 : 1;
    // expected steps between two references of a row = rows / references per step
    if (q.f.lazy_adam) a.long_gap = (U->rows / B > 64 || V->rows / (2 * B) > 64) && getenv("ORX_ADAM_NO_LONGGAP") == nullptr;
    if (q.f.fused_censor) { CHECK(orx_table_side(V)); a.censor = 1; a.min_norm = 0.1f; a.sideV = V->side; }
    q.launch = [&p](int64_t s, int64_t) -> int {
        ExactCall& q = p.q;
        q.a.wt = p.dw ? p.dw + s * q.ds : nullptr;      // (the caller's order: the kernel reads it at the triplet's original position)
        return orx_launch_fused(q.c, p.kmodel, q.opt->kind, q.f.mode, q.a);
    };
    if (q.f.censor) {
        q.flags = [&q](int64_t s0, int64_t kc) -> int { return pair_censor_flags(q, s0, kc); };
        q.after_step = [&q](int64_t s0, int64_t i, int64_t kc) -> int { return pair_censor_step(q, s0, i, kc); };
    }
    return exact_run(q, PAIR_TRAITS, flags, loss_out, l2_out);
}

extern "C" int orx_pairwise_reserve(orx_ctx* c, orx_opt* opt, orx_table* U, orx_table* V, orx_table* b, int64_t K, int64_t B) {
    ORX_ARG(c && opt, "orx_pairwise_reserve: NULL context/optimizer");
    CHECK(check_pair_tables(U, V, b));
    ORX_ARG(K > 0 && B > 0, "orx_pairwise_reserve: K and B must be positive");
    ORX_HIP(hipSetDevice(c->device));
    ExactCall q;
    q.c = c; q.opt = opt; q.U = U; q.V = V; q.b = b; q.K = K; q.B = B;
    q.np = orx_fused_nwaves(U->dim, B);
    q.f = exact_form(PAIR_TRAITS, opt, U, V, b, K, 0, 0);
    CHECK(exact_reserve(q, PAIR_TRAITS, orx_pairing_wanted(q.f.mode, q.f.role_bits, opt->kind, U->dim, B, 0)));
    ORX_HIP(hipStreamSynchronize(c->stream));
    return ORX_OK;
}

extern "C" int orx_pairwise_loss(orx_ctx* c, int model, orx_table* U, orx_table* V, orx_table* b,
                                 const int32_t* uid, const int32_t* pid, const int32_t* nid,
                                 int64_t B, float margin, int flags, float* loss_out, float* l2_out) {
    return orx_pairwise_loss_impl(c, model, U, V, b, uid, pid, nid, nullptr, B, margin, flags, loss_out, l2_out);
}

int orx_pairwise_loss_impl(orx_ctx* c, int model, orx_table* U, orx_table* V, orx_table* b,
                           const int32_t* uid, const int32_t* pid, const int32_t* nid, const float* weight,
                           int64_t B, float margin, int flags, float* loss_out, float* l2_out) {
    CHECK(orx_sync_tables({U, V, b}));
    ORX_ARG(c, "orx_pairwise_loss: NULL context");
    ORX_ARG(model == ORX_BPR || model == ORX_UCML, "orx_pairwise_loss: unknown model %d", model);
    CHECK(check_pair_tables(U, V, b, model, flags));
    ORX_ARG(B > 0 && uid && pid && nid, "orx_pairwise_loss: empty batch or NULL ids");
    ORX_HIP(hipSetDevice(c->device));
    StepInputs in;
    CHECK(orx_stage_steps(c, 1, B, B, flags, {{uid, 1}, {pid, 1}, {nid, 1}}, {{weight, 1}}, &in));
    return orx_run_forward(c, orx_fused_nwaves(U->dim, B), loss_out, l2_out, [&](float* partial) -> int {
        PairArgs a;
        memset(&a, 0, sizeof(a));
        a.U = U->w; a.V = V->w; a.b = b ? b->w : nullptr;
        a.B = B; a.NU = U->rows; a.NI = V->rows; a.D = U->dim;
        a.margin = margin; a.invB = 1.0f / (float)B; a.l2w = 1.f;
        a.partial = partial; a.err = c->d_err;
        a.uid = in.id[0]; a.pid = in.id[1]; a.nid = in.id[2]; a.wt = in.f[0];
        return orx_launch_fused(c, b ? model : MODEL_BPR_NB, ORX_SGD, MODE_LOSS, a);
    });
}

// ------------------------------------------------------------ pointwise (GMF / WRMF) ---
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

// PointArgs from the driver's view of the tables: everything the two layouts share, for the call or -- the fields exact_step sets -- for a step
static void point_from_view(const PairArgs& v, PointArgs* a) {
    a->U = v.U; a->V = v.V; a->b = v.b; a->gU = v.gU; a->gV = v.gV; a->gb = v.gb; a->aU = v.aU; a->aV = v.aV; a->ab = v.ab;
    a->role_bits = v.role_bits; a->gU2 = v.gU2; a->gV2 = v.gV2; a->gb2 = v.gb2; a->readyU = v.readyU; a->readyV = v.readyV;
    a->B = v.B; a->NU = v.NU; a->NI = v.NI; a->D = v.D; a->lr = v.lr; a->eps = v.eps; a->invB = v.invB; a->err = v.err;
    a->a2U = v.a2U; a->a2V = v.a2V; a->a2b = v.a2b; a->lastU = v.lastU; a->lastV = v.lastV; a->lastb = v.lastb;
    a->lrt = v.lrt; a->b1 = v.b1; a->b2 = v.b2; a->newton = v.newton; a->lrv = v.lrv; a->cf_delta = v.cf_delta; a->cf_lb1 = v.cf_lb1; a->cf_lb2 = v.cf_lb2;
    a->uid = v.uid; a->iid = v.pid; a->ids4 = v.ids4;      // (with pairing the SoA copy is not written: the records are the input)
    a->refinfo = v.refinfo; a->segstart = v.segstart; a->stage = v.stage; a->stageb = v.stageb;
    a->partial = v.partial; a->step_t = v.step_t; a->epoch = v.epoch; a->n_apply_blocks = v.n_apply_blocks;
}

struct PointStep {
    ExactCall q; int model; orx_table* w; OptSlots sw; PointArgs a;
    int nw;                 // loss partials of the samples; GMF: one more slot for 0.5 * ||w||^2
    bool dense_tail;        // GMF on the float4 kernels: the Dense(1) gradient is reduced and applied by the last workgroups of the step's own launch
};

// exact mode without role bits (tables >= 2^28 rows, generic dims): byte flags + atomics for every duplicate
static int point_byte_flags(PointStep& p, int64_t s0, int64_t kc) {
    ExactCall& q = p.q; orx_ctx* c = q.c;
    const int64_t B = q.B, list_stride = 2 * B;
    ENSURE(c->d_dflag, c->d_dflag_cap, (size_t)kc * 2 * B);
    ENSURE(c->d_dlist, c->d_dlist_cap, (size_t)kc * list_stride * sizeof(uint32_t));
    ENSURE(c->d_dcount, c->d_dcount_cap, (size_t)kc * sizeof(int));
    DedupArgs d;
    memset(&d, 0, sizeof(d));
    d.uid = q.ids[0] + s0 * q.ds; d.pid = d.nid = q.ids[1] + s0 * q.ds; d.id_stride = q.ds;
    d.dflag = c->d_dflag; d.dlist = c->d_dlist; d.dcount = c->d_dcount;
    d.flag_stride = 2 * B; d.list_stride = list_stride;
    d.nU = B; d.nP = B; d.nN = 0; d.NU = q.U->rows; d.NI = q.V->rows;
    d.nbu = orx_dedup_buckets(q.U->rows); d.nbi = orx_dedup_buckets(q.V->rows);
    ORX_HIP(hipMemsetAsync(c->d_dcount, 0, (size_t)kc * sizeof(int), c->stream));
    return orx_launch_dedup(c, d, kc);
}

static int point_launch(PointStep& p, int64_t s, int64_t i) {
    ExactCall& q = p.q;
    PointArgs& a = p.a;
    point_from_view(q.a, &a);
    a.label = q.label + s * q.ds;
    a.wt_l2slot = a.partial + 2 * p.nw;
    if (!q.f.plan) a.dflag = q.c->d_dflag + (size_t)i * 2 * q.B;
    if (a.n_apply_blocks) a.ap = q.a;      // this launch also applies the duplicated rows of step i - 1
    return orx_launch_point_fused(q.c, p.model, q.opt->kind, q.f.mode, a);
}

// GMF's dense Dense(1) kernel: reduce the partials, apply the dense rule
static int gmf_dense_step(PointStep& p) {
    ExactCall& q = p.q; orx_ctx* c = q.c; orx_opt* opt = q.opt; orx_table* w = p.w;
    const PointArgs& a = p.a;
    if (q.f.mode == MODE_ACCUM || q.f.lazy_adam) {
        const float lr_t = q.f.lazy_adam ? opt->h_lrt[(size_t)opt->t] : q.lr_t;
        if (!p.dense_tail) CHECK(orx_launch_dense_reduce(c, c->d_wpart, orx_point_wparts(a.D, a.B), a.D, w->w, a.l2w, w->gsum, a.wt_l2slot, nullptr, -1, 0.f, 0.f));
        return orx_launch_adam_sweep(c, w->w, p.sw.s0, p.sw.s1, w->gsum, a.D, lr_t, opt->p0, opt->p1, opt->p2);
    }
    if (p.dense_tail) return ORX_OK;
    // reduce + dense SGD / Adagrad rule in one launch
    return orx_launch_dense_reduce(c, c->d_wpart, orx_point_wparts(a.D, a.B), a.D, w->w, a.l2w, nullptr, a.wt_l2slot, p.sw.s0, opt->kind, opt->lr, a.eps);
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
    ht_mark("enter", true);
    ORX_HIP(hipSetDevice(c->device));
    PointStep p;
    ExactCall& q = p.q;
    q.c = c; q.opt = opt; q.U = U; q.V = V; q.b = b; q.K = K; q.B = B;
    p.model = model; p.w = w;
    StepInputs in;
    CHECK(orx_stage_steps(c, K, B, id_stride, flags, {{uid, 1}, {iid, 1}}, {{label, 1}}, &in));
    q.ids[0] = in.id[0]; q.ids[1] = q.ids[2] = in.id[1]; q.nN = 0; q.label = in.f[0]; q.ds = in.ds;
    ORX_ARG(!(flags & ORX_HOGWILD) || opt->kind != ORX_MOMENTUM, "orx_pointwise_step: ORX_HOGWILD is not supported with momentum (its racy in-place pass has no velocity rule)");
    const int fb = orx_fallback_bits();
    // TF-2.0 Adam applied lazily, as in orx_pairwise_step: float4 dims with the exact-step plan; the
    // Dense(1) kernel of GMF is a dense parameter and takes the plain rule.  Otherwise every reference accumulates
    // and the tables are swept whole.
    q.f = exact_form(POINT_TRAITS, opt, U, V, b, K, flags & ORX_HOGWILD, fb);
    const int D = U->dim;
    p.nw = orx_point_nwaves(D, B);
    q.np = p.nw + (model == ORX_GMF ? 1 : 0);
    q.want_loss = true;         // (no loss-free form of these kernels: the sums are always launched)
    CHECK(exact_prepare(q, POINT_TRAITS, model, false, fb));
    if (w) { CHECK(orx_table_sync(w)); CHECK(orx_table_scratch(w)); CHECK(orx_opt_slots(opt, w, &p.sw)); }
    if (model == ORX_GMF) ENSURE(c->d_wpart, c->d_wpart_cap, (size_t)(p.nw + 256) * D * sizeof(float));   // + stage-1 rows of dense_reduce
    CHECK(exact_view(q));
    PointArgs& a = p.a;
    memset(&a, 0, sizeof(a));
    a.w = w ? w->w : nullptr;
    a.l2w = l2w; a.a_w = a_w; a.b_w = b_w;
    a.sigmoid = (model == ORX_WRMF && (flags & ORX_POINT_SIGMOID)) ? 1 : 0;
    a.wpartial = c->d_wpart;
    p.dense_tail = model == ORX_GMF && orx_point_dense_tail_ok(D);
    if (p.dense_tail) {
        // the partial rows and the group rows behind them start out EMPTY (all ones); every launch hands them back that way
        const size_t nrows = (size_t)orx_point_wparts(D, B) + (size_t)orx_point_reducers(D, B) - 1;
        ORX_HIP(hipMemsetAsync(c->d_wpart, 0xff, nrows * D * sizeof(float), c->stream));
        a.wt_nred = orx_point_reducers(D, B); a.wt_rows = c->d_wpart + (size_t)orx_point_wparts(D, B) * D;
        const bool to_gout = q.f.mode == MODE_ACCUM || q.f.lazy_adam;                        // (Adam: adam_sweep_kernel applies the gradient)
        a.wt_gout = to_gout ? w->gsum : nullptr; a.wt_acc = to_gout ? nullptr : p.sw.s0; a.wt_optkind = to_gout ? -1 : opt->kind;
    }
    q.launch = [&p](int64_t s, int64_t i) -> int { return point_launch(p, s, i); };
    if (q.f.mode == MODE_EXACT && !q.f.plan) q.flags = [&p](int64_t s0, int64_t kc) -> int { return point_byte_flags(p, s0, kc); };
    if (model == ORX_GMF) q.after_step = [&p](int64_t, int64_t, int64_t) -> int { return gmf_dense_step(p); };
    return exact_run(q, POINT_TRAITS, flags, loss_out, l2_out);
}

extern "C" int orx_pointwise_loss(orx_ctx* c, int model, orx_table* U, orx_table* V, orx_table* b, orx_table* w,
                                  const int32_t* uid, const int32_t* iid, const float* label,
                                  int64_t B, float a_w, float b_w, int flags, float* loss_out, float* l2_out) {
    CHECK(orx_sync_tables({U, V, b, w}));
    ORX_ARG(c, "orx_pointwise_loss: NULL context");
    CHECK(check_point_tables(model, U, V, b, w));
    ORX_ARG(B > 0 && uid && iid && label, "orx_pointwise_loss: empty batch or NULL pointer");
    ORX_HIP(hipSetDevice(c->device));
    StepInputs in;
    CHECK(orx_stage_steps(c, 1, B, B, flags, {{uid, 1}, {iid, 1}}, {{label, 1}}, &in));
    const int D = U->dim, nw = orx_point_nwaves(D, B);
    return orx_run_forward(c, nw + (model == ORX_GMF ? 1 : 0), loss_out, l2_out, [&](float* partial) -> int {
        PointArgs a;
        memset(&a, 0, sizeof(a));
        a.U = U->w; a.V = V->w; a.b = b->w; a.w = w ? w->w : nullptr;
        a.B = B; a.NU = U->rows; a.NI = V->rows; a.D = D;
        a.invB = 1.0f / (float)B; a.l2w = 1.f; a.a_w = a_w; a.b_w = b_w;
        a.sigmoid = (model == ORX_WRMF && (flags & ORX_POINT_SIGMOID)) ? 1 : 0;
        a.partial = partial; a.err = c->d_err;
        a.uid = in.id[0]; a.iid = in.id[1]; a.label = in.f[0];
        CHECK(orx_launch_point_fused(c, model, ORX_SGD, MODE_LOSS, a));
        // GMF: the 0.5 * ||w||^2 slot behind the samples' partials
        return model == ORX_GMF ? orx_launch_dense_reduce(c, nullptr, 0, D, w->w, 0.f, nullptr, partial + 2 * nw, nullptr, -1, 0.f, 0.f) : ORX_OK;
    });
}
