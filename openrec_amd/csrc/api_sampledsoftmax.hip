// The sampled softmax over a shared candidate list: the checks, the scratch layout, the staging of host lists and the driver of
// every call on this objective, and the C-ABI entry points orx_sampled_softmax_step / _loss / _geometry (the user-table form) and
// orx_seqrec_sampled_step / _loss (the bag form).  include/openrec_hip.h has the semantics, kernels_sampledsoftmax.hip the
// kernels (kernels_sampledsoftmax16.hip those under ORX_SS_BF16); the query comes from a FullSoftmaxForm (orx_internal.h), built
// by the builders the full softmax's entry points use.
//
// Per step: a table outside the mask is finished first, every other one stays lazy; the form touches its rows and writes Q; the
// rows of V and b under pid and cand are touched; gather, the row kernel, [the column kernel and its finish]; [Adam: the counter
// advances]; the form's apply; one sort of the B + S item rows (labels, then candidates) and the sparse rule on the item table and
// on the bias with it.  No kernel before the applies writes a table, so every gradient is taken on the pre-step tables.  The
// scratch of a step is carved from the context's grow-only d_tmp and reused by every step.
#include <cmath>
#include <cstring>

#include "orx_internal.h"

namespace {

struct Layout {
    SampledSoftmaxPlan plan;
    size_t cand, coff, xq, xp, xc, key, cw, sq, pb, po, ckey, cb, co, rmax, cn, rowloss, list, gpc, bpc, gu, gi, sorted;
    size_t xq16, xc16, spos, apos, pm, pE, gqc;             // ORX_SS_BF16
};

int check_shape(const char* fn, int64_t B, int64_t S, int32_t D, float scale) {
    ORX_ARG(D >= 1 && D <= 256, "%s: dim %d outside [1, 256]", fn, D);
    ORX_ARG(std::isfinite(scale) && scale > 0.f, "%s: scale must be finite and > 0 (got %g)", fn, (double)scale);
    ORX_ARG(B >= 0 && B <= 0x7fff0000LL, "%s: B = %lld (B + S must fit 31 bits)", fn, (long long)B);
    ORX_ARG(S >= 0 && S <= 65536, "%s: S = %lld candidates (0 <= S <= 65536)", fn, (long long)S);
    return ORX_OK;
}

int check_flags(const char* fn, int flags) {
    ORX_ARG((flags & ~(ORX_IDS_DEVICE | ORX_SS_MASK_HITS | ORX_SS_BF16)) == 0, "%s: flags other than ORX_IDS_DEVICE | ORX_SS_MASK_HITS | ORX_SS_BF16 (0x%x)", fn, flags);
    return ORX_OK;
}

// host_cand / host_coff: a piece for the host list; grads: the step's buffers, query_side / item_side the two gradient sides';
// bf16: ORX_SS_BF16 -- the bf16 copies in the place of the candidates' fp32 copy, and what the split row side passes on
void layout(Carve* cv, int64_t B, int64_t S, int32_t D, bool host_cand, bool host_coff, bool grads, bool query_side, bool item_side, bool bf16, Layout* l) {
    memset(l, 0, sizeof(*l));
    SampledSoftmaxPlan& p = l->plan;
    if (bf16) orx_sampledsoftmax16_plan(B, S, D, &p); else orx_sampledsoftmax_plan(B, S, D, &p);
    const int gs = (D + 1 + 3) & ~3;
    const size_t row = (size_t)p.Bp * sizeof(float), rows = row * p.Dp, col = (size_t)p.Sp * sizeof(float), cols = col * p.Dp;
    if (host_cand) l->cand = cv->take((size_t)S * sizeof(int32_t));
    if (host_coff) l->coff = cv->take((size_t)S * sizeof(float));
    l->xq = cv->take(rows); l->xp = cv->take(rows);
    if (bf16) {
        l->xq16 = cv->take((size_t)p.Bp * p.Dk * sizeof(unsigned short)); l->xc16 = cv->take((size_t)p.Sp * p.Dk * sizeof(unsigned short));
        l->spos = cv->take(row); l->apos = cv->take(row);
        l->pm = cv->take(row * p.ncc); l->pE = cv->take(row * p.ncc);
        if (grads && query_side) l->gqc = cv->take(rows * p.ncc);
    } else {
        l->xc = cv->take(cols);
    }
    l->key = cv->take(row); l->cw = cv->take(row); l->sq = cv->take(row); l->pb = cv->take(row); l->po = cv->take(row);
    l->ckey = cv->take(col); l->cb = cv->take(col); l->co = cv->take(col);
    l->rmax = cv->take(row); l->cn = cv->take(row); l->rowloss = cv->take(row);
    if (grads && query_side) l->gu = cv->take((size_t)B * gs * sizeof(float));
    if (grads && item_side) {
        l->list = cv->take((size_t)(B + S) * sizeof(int32_t));
        l->gpc = cv->take(cols * p.ncs); l->bpc = cv->take(col * p.ncs);
        l->gi = cv->take((size_t)(B + S) * gs * sizeof(float));
        l->sorted = cv->take((size_t)(B + S) * sizeof(uint2));
    }
}

struct Call {
    orx_table* V; orx_table* b;
    const int32_t* pid; const int32_t* cand; const float* weight; const float* pos_offset; const float* cand_offset;
    int64_t B; int64_t S; float scale; int flags;
};

// what a step and a forward share once their checks have passed: the lists on the device, the scratch of the form and of the
// objective in d_tmp, the kernels' arguments (partial is the caller's to set) and the FullSoftmaxArgs the form's members read
int prepare(orx_ctx* c, FullSoftmaxForm& f, const Call& k, float l2w, bool grads, bool item_side, SampledSoftmaxArgs* out, FullSoftmaxArgs* fa,
            uint2** sorted) {
    ORX_ARG(k.pid && (k.S == 0 || k.cand) && (!f.has_ids || f.ids), "%s: NULL id pointer", f.fn);
    ORX_HIP(hipSetDevice(c->device));
    const bool host = !(k.flags & ORX_IDS_DEVICE);
    orx_table* V = k.V;
    StepInputs in;
    if (f.has_ids) CHECK(orx_stage_steps(c, 1, k.B, k.B, k.flags, {{f.ids, 1}, {k.pid, 1}}, {{k.weight, 1}, {k.pos_offset, 1}}, &in));
    else CHECK(orx_stage_steps(c, 1, k.B, k.B, k.flags, {{k.pid, 1}}, {{k.weight, 1}, {k.pos_offset, 1}}, &in));
    Carve cv;
    f.carve(&cv, grads);
    Layout l;
    const bool bf16 = (k.flags & ORX_SS_BF16) != 0;
    layout(&cv, k.B, k.S, V->dim, host && k.S, host && k.S && k.cand_offset, grads, grads && f.query_side, item_side, bf16, &l);
    ENSURE(c->d_tmp, c->d_tmp_cap, cv.off);
    FullSoftmaxQuery q;
    memset(&q, 0, sizeof(q));
    q.qid = f.has_ids ? in.id[0] : nullptr;
    CHECK(f.bind(grads, &q));
    char* base = reinterpret_cast<char*>(c->d_tmp);
    auto fp = [&](size_t o) { return reinterpret_cast<float*>(base + o); };
    auto ip = [&](size_t o) { return reinterpret_cast<int32_t*>(base + o); };
    SampledSoftmaxArgs a;
    memset(&a, 0, sizeof(a));
    const SampledSoftmaxPlan& p = l.plan;
    a.Q = q.Q; a.V = V->w; a.b = k.b ? k.b->w : nullptr;
    a.qid = q.qid; a.pid = in.id[f.has_ids ? 1 : 0]; a.wt = in.f[0]; a.poff = in.f[1];
    a.cand = k.cand; a.coff = k.cand_offset;
    if (host && k.S) {                          // the two lists of S entries live where the ids live
        ORX_HIP(hipMemcpyAsync(ip(l.cand), k.cand, (size_t)k.S * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        a.cand = ip(l.cand);
        if (k.cand_offset) {
            ORX_HIP(hipMemcpyAsync(fp(l.coff), k.cand_offset, (size_t)k.S * sizeof(float), hipMemcpyHostToDevice, c->stream));
            a.coff = fp(l.coff);
        }
    }
    a.B = k.B; a.Bp = p.Bp; a.NQ = q.NQ; a.NI = V->rows; a.S = k.S; a.Sp = p.Sp;
    a.D = V->dim; a.Dp = (int)p.Dp; a.gs = (a.D + 1 + 3) & ~3; a.ncs = (int)p.ncs; a.tps = (int)p.tps;
    a.mask = (k.flags & ORX_SS_MASK_HITS) ? 1 : 0;
    a.scale = k.scale; a.invB = 1.0f / (float)k.B; a.l2w = l2w; a.err = c->d_err;
    a.xq = fp(l.xq); a.xp = fp(l.xp);
    if (bf16) {
        a.xq16 = reinterpret_cast<unsigned short*>(base + l.xq16); a.xc16 = reinterpret_cast<unsigned short*>(base + l.xc16);
        a.Dk = (int)p.Dk; a.ncc = (int)p.ncc; a.tpc = (int)p.tpc;
        a.spos = fp(l.spos); a.apos = fp(l.apos); a.pm = fp(l.pm); a.pE = fp(l.pE);
        if (grads && f.query_side) a.gqc = fp(l.gqc);
    } else {
        a.xc = fp(l.xc);
    }
    a.key = ip(l.key); a.cw = fp(l.cw); a.sq = fp(l.sq); a.pb = fp(l.pb); a.po = fp(l.po);
    a.ckey = ip(l.ckey); a.cb = fp(l.cb); a.co = fp(l.co);
    a.rmax = fp(l.rmax); a.cn = fp(l.cn); a.rowloss = fp(l.rowloss);
    if (grads && f.query_side) a.gu = fp(l.gu);
    if (grads && item_side) { a.list = ip(l.list); a.gpc = fp(l.gpc); a.bpc = fp(l.bpc); a.gi = fp(l.gi); *sorted = reinterpret_cast<uint2*>(base + l.sorted); }
    *out = a;
    memset(fa, 0, sizeof(*fa));                 // what the form's produce and apply read of the full softmax's arguments
    fa->Q = a.Q; fa->V = a.V; fa->b = a.b; fa->qid = a.qid; fa->pid = a.pid; fa->wt = a.wt;
    fa->B = a.B; fa->Bp = a.Bp; fa->NQ = a.NQ; fa->NI = a.NI; fa->D = a.D; fa->Dp = a.Dp; fa->gs = a.gs;
    fa->scale = a.scale; fa->invB = a.invB; fa->l2w = fa->l2q = l2w; fa->gu = a.gu; fa->err = a.err;
    return ORX_OK;
}

int touch_items(const Call& k, const SampledSoftmaxArgs& a) {
    return orx_touch_step(nullptr, k.V, k.b, nullptr, 0, a.pid, k.B, k.S ? a.cand : nullptr, k.S);
}

int drive_step(orx_ctx* c, orx_opt* opt, FullSoftmaxForm& f, const Call& k, float l2_reg, int train_mask, float* loss_out, float* l2_out) {
    const char* fn = f.fn;
    orx_table* V = k.V; orx_table* b = k.b;
    CHECK(check_flags(fn, k.flags));
    CHECK(f.check());
    CHECK(check_shape(fn, k.B, k.S, V->dim, k.scale));
    CHECK(f.train(&train_mask));
    for (int i = 0; i < f.n_tab; ++i)
        if (!f.tab[i].dense) CHECK(orx_check_apply_rows_opt(opt, f.tab[i].t, nullptr));
    CHECK(orx_check_apply_rows_opt(opt, V, nullptr));
    if (k.B == 0) return ORX_OK;
    const bool tV = (train_mask & ORX_TRAIN_ITEM) != 0, tb = (train_mask & ORX_TRAIN_BIAS) != 0;
    SampledSoftmaxArgs a;
    FullSoftmaxArgs fa;
    uint2* sorted = nullptr;
    CHECK(prepare(c, f, k, l2_reg, true, tV || tb, &a, &fa, &sorted));
    // a table outside the mask is finished under the old counter (whatever optimizer it is lazy under), then only read; the item
    // table and the bias are read by rows here, so inside the mask they stay lazy
    orx_table* keep[2 + sizeof(f.tab) / sizeof(f.tab[0])]; int n_keep = 0;
    for (int i = 0; i < f.n_tab; ++i) { if (f.tab[i].trained) keep[n_keep++] = f.tab[i].t; else CHECK(orx_table_sync(f.tab[i].t)); }
    if (tV) keep[n_keep++] = V; else CHECK(orx_table_sync(V));
    if (b) { if (tb) keep[n_keep++] = b; else CHECK(orx_table_sync(b)); }
    const int64_t n_rows = k.B + k.S;

    const int rc = orx_run_steps(c, 1, orx_sampledsoftmax_npartials(k.B), k.flags, loss_out, l2_out, nullptr, [&](int64_t, int64_t, float* partial) -> int {
        a.partial = partial;
        CHECK(f.produce(fa, true));
        CHECK(touch_items(k, a));
        if (k.flags & ORX_SS_BF16) {
            CHECK(orx_launch_sampledsoftmax16_forward(c, a));
            CHECK(orx_launch_sampledsoftmax16_grads(c, a));
        } else {
            CHECK(orx_launch_sampledsoftmax_rows(c, a, f.query_side));
            if (tV || tb) CHECK(orx_launch_sampledsoftmax_cols(c, a));
        }
        if (opt->kind == ORX_ADAM) CHECK(orx_opt_advance(opt, keep, n_keep));      // once per step: after the step's reads, before its applies
        CHECK(f.apply(fa));
        if (tV || tb) {                         // one sort of pid | cand, each table on its own: a row's occurrences are summed in list order
            CHECK(orx_rows_sort_keep(c, a.list, 1, n_rows, n_rows, V->rows, sorted));
            if (tV) CHECK(orx_apply_rows_sorted(c, opt, V, sorted, n_rows, a.gi, a.gs));
            if (tb) CHECK(orx_apply_rows_sorted(c, opt, b, sorted, n_rows, a.gi + a.D, a.gs));
        }
        return ORX_OK;
    });
    CHECK(rc);
    // device lists whose caller took the losses: the call has synchronised, so the index flag is looked at here as well
    if ((k.flags & ORX_IDS_DEVICE) && (loss_out || l2_out)) return orx_check_index_error(c);
    return ORX_OK;
}

int drive_loss(orx_ctx* c, FullSoftmaxForm& f, const Call& k, float* loss_out, float* l2_out, float* row_loss_out) {
    const char* fn = f.fn;
    CHECK(check_flags(fn, k.flags));
    CHECK(f.check());
    CHECK(check_shape(fn, k.B, k.S, k.V->dim, k.scale));
    if (k.B == 0) {
        if (loss_out) *loss_out = 0.f;
        if (l2_out) *l2_out = 0.f;
        return ORX_OK;
    }
    SampledSoftmaxArgs a;
    FullSoftmaxArgs fa;
    CHECK(prepare(c, f, k, 0.f, false, false, &a, &fa, nullptr));
    const bool host = !(k.flags & ORX_IDS_DEVICE);
    return orx_run_forward(c, orx_sampledsoftmax_npartials(k.B), loss_out, l2_out, [&](float* partial) -> int {
        a.partial = partial;
        CHECK(f.produce(fa, false));
        CHECK(touch_items(k, a));
        if (k.flags & ORX_SS_BF16) CHECK(orx_launch_sampledsoftmax16_forward(c, a));
        else CHECK(orx_launch_sampledsoftmax_rows(c, a, false));
        if (row_loss_out)
            ORX_HIP(hipMemcpyAsync(row_loss_out, a.rowloss, (size_t)k.B * sizeof(float), host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
        return ORX_OK;
    });
}

}  // namespace

extern "C" int orx_sampled_softmax_geometry(int64_t B, int64_t S, int32_t D, int64_t out[5]) {
    static const char* fn = "orx_sampled_softmax_geometry";
    ORX_ARG(out, "%s: NULL out", fn);
    CHECK(check_shape(fn, B, S, D, 1.0f));
    Carve cv;
    Layout l;
    layout(&cv, B, S, D, false, false, true, true, true, false, &l);
    out[0] = 64; out[1] = 64; out[2] = l.plan.ncs; out[3] = l.plan.Dp; out[4] = (int64_t)cv.off;
    return ORX_OK;
}

extern "C" int orx_sampled_softmax_bf16_geometry(int64_t B, int64_t S, int32_t D, int64_t out[6]) {
    static const char* fn = "orx_sampled_softmax_bf16_geometry";
    ORX_ARG(out, "%s: NULL out", fn);
    CHECK(check_shape(fn, B, S, D, 1.0f));
    Carve cv;
    Layout l;
    layout(&cv, B, S, D, false, false, true, true, true, true, &l);
    out[0] = 64; out[1] = 64; out[2] = l.plan.ncs; out[3] = l.plan.ncc; out[4] = l.plan.Dk; out[5] = (int64_t)cv.off;
    return ORX_OK;
}

extern "C" int orx_sampled_softmax_step(orx_ctx* c, orx_opt* opt, orx_table* U, orx_table* V, orx_table* b,
                                        const int32_t* uid, const int32_t* pid, const int32_t* cand,
                                        const float* weight, const float* pos_offset, const float* cand_offset,
                                        int64_t B, int64_t S, float scale, float l2_reg, int train_mask, int flags,
                                        float* loss_out, float* l2_out) {
    static const char* fn = "orx_sampled_softmax_step";
    CHECK(check_flags(fn, flags));
    auto f = orx_fullsoftmax_user_form(fn, true, c, opt, U, V, b, uid, B, l2_reg, flags & ORX_IDS_DEVICE);
    return drive_step(c, opt, *f, Call{V, b, pid, cand, weight, pos_offset, cand_offset, B, S, scale, flags}, l2_reg, train_mask, loss_out, l2_out);
}

extern "C" int orx_sampled_softmax_loss(orx_ctx* c, orx_table* U, orx_table* V, orx_table* b,
                                        const int32_t* uid, const int32_t* pid, const int32_t* cand,
                                        const float* weight, const float* pos_offset, const float* cand_offset,
                                        int64_t B, int64_t S, float scale, int flags, float* loss_out, float* l2_out, float* row_loss_out) {
    static const char* fn = "orx_sampled_softmax_loss";
    CHECK(check_flags(fn, flags));
    auto f = orx_fullsoftmax_user_form(fn, false, c, nullptr, U, V, b, uid, B, 0.f, flags & ORX_IDS_DEVICE);
    return drive_loss(c, *f, Call{V, b, pid, cand, weight, pos_offset, cand_offset, B, S, scale, flags}, loss_out, l2_out, row_loss_out);
}

extern "C" int orx_seqrec_sampled_step(orx_ctx* c, orx_opt* opt, orx_table* hist, orx_table* item, orx_table* b,
                                       const int32_t* bag_ptr, const int32_t* bag_items, const int32_t* pid, const int32_t* cand,
                                       const float* weight, const float* pos_offset, const float* cand_offset,
                                       int64_t B, int64_t n, int64_t S, int mode, float denom, float scale, float l2_reg, int train_mask, int flags,
                                       float* loss_out, float* l2_out) {
    static const char* fn = "orx_seqrec_sampled_step";
    CHECK(check_flags(fn, flags));
    auto f = orx_seqrec_bag_form(fn, true, c, opt, hist, item, b, bag_ptr, bag_items, B, n, mode, denom, l2_reg, flags & ORX_IDS_DEVICE);
    return drive_step(c, opt, *f, Call{item, b, pid, cand, weight, pos_offset, cand_offset, B, S, scale, flags}, l2_reg, train_mask, loss_out, l2_out);
}

extern "C" int orx_seqrec_sampled_loss(orx_ctx* c, orx_table* hist, orx_table* item, orx_table* b,
                                       const int32_t* bag_ptr, const int32_t* bag_items, const int32_t* pid, const int32_t* cand,
                                       const float* weight, const float* pos_offset, const float* cand_offset,
                                       int64_t B, int64_t n, int64_t S, int mode, float denom, float scale, int flags,
                                       float* loss_out, float* l2_out, float* row_loss_out) {
    static const char* fn = "orx_seqrec_sampled_loss";
    CHECK(check_flags(fn, flags));
    auto f = orx_seqrec_bag_form(fn, false, c, nullptr, hist, item, b, bag_ptr, bag_items, B, n, mode, denom, 0.f, flags & ORX_IDS_DEVICE);
    return drive_loss(c, *f, Call{item, b, pid, cand, weight, pos_offset, cand_offset, B, S, scale, flags}, loss_out, l2_out, row_loss_out);
}
