// The softmax over all items: the two host drivers every call on this objective goes through (orx_fullsoftmax_drive_step /
// orx_fullsoftmax_drive_loss; orx_internal.h has the query form they take), the checks, scratch layout and bind of the objective
// and of the label sets, and the C-ABI entry points of the user-table form: orx_fullsoftmax_step, orx_fullsoftmax_loss and
// orx_fullsoftmax_geometry (include/openrec_hip.h has the semantics, kernels_fullsoftmax.hip and kernels_labelsets.hip the
// kernels; the bag form is in api_seqrec.hip, the tower form in api_tower.hip).
//
// Per step: the item table, the bias and the form's dense tables are read in full, so a lazily applied Adam on them is finished
// first and they leave the lazy set; the form touches its rows and writes Q; the forward and the gradient passes; the form's
// backward; [Adam: the counter advances]; the form's applies, then the DENSE rule of the optimizer on the item table and the bias
// (orx_table_apply_dense_at: every row has a gradient).  No kernel before the applies writes a table, so every gradient is taken
// on the pre-step tables.  The scratch of a step is carved from the context's grow-only d_tmp and reused by every step.
#include <cmath>
#include <cstring>

#include "orx_graph.h"
#include "orx_internal.h"

namespace {

constexpr int FS_FLAGS = ORX_IDS_DEVICE | ORX_NO_L2 | ORX_HOGWILD | ORX_CENSOR;      // (the last two are named to be refused by name)

}  // namespace

int orx_fullsoftmax_check(const char* fn, int64_t B, int64_t NI, int32_t D, float scale, int32_t chunk_items, int32_t chunk_samples) {
    ORX_ARG(D >= 1 && D <= 256, "%s: dim %d outside [1, 256]", fn, D);
    ORX_ARG(std::isfinite(scale) && scale > 0.f, "%s: scale must be finite and > 0 (got %g)", fn, (double)scale);
    ORX_ARG(chunk_items >= 0 && chunk_items % 64 == 0, "%s: chunk_items must be 0 or a positive multiple of the tile width 64 (got %d)", fn, chunk_items);
    ORX_ARG(chunk_samples >= 0 && chunk_samples % 64 == 0, "%s: chunk_samples must be 0 or a positive multiple of the tile width 64 (got %d)", fn, chunk_samples);
    ORX_ARG(B >= 0 && B <= 0x7fffff00LL, "%s: B = %lld (B must fit 31 bits)", fn, (long long)B);
    ORX_ARG(NI >= 1 && NI <= 0x7fffff00LL, "%s: %lld items (the item count must fit 31 bits)", fn, (long long)NI);
    FullSoftmaxPlan p;
    orx_fullsoftmax_plan(B, NI, D, chunk_items, chunk_samples, &p);
    ORX_ARG(p.nci <= 65535 && p.ncs <= 65535, "%s: %lld item chunks and %lld sample chunks (at most 65535 each: raise the chunk size)", fn,
            (long long)p.nci, (long long)p.ncs);
    ORX_ARG(p.NIp * p.Dp < 0xffffff00LL, "%s: %lld items of padded dim %lld: the padded copy of the item table is indexed by 32 bits", fn,
            (long long)NI, (long long)p.Dp);
    return ORX_OK;
}

void orx_fullsoftmax_layout(Carve* cv, int64_t B, int64_t NI, int32_t D, int32_t chunk_items, int32_t chunk_samples, bool grads, bool query_side,
                            bool item_side, bool host_off, FullSoftmaxLayout* l) {
    memset(l, 0, sizeof(*l));
    FullSoftmaxPlan& p = l->plan;
    orx_fullsoftmax_plan(B, NI, D, chunk_items, chunk_samples, &p);
    const int gs = (D + 1 + 3) & ~3;
    const size_t row = (size_t)p.Bp * sizeof(float), rows = (size_t)p.Bp * p.Dp * sizeof(float);
    const size_t irow = (size_t)p.NIp * sizeof(float), irows = (size_t)p.NIp * p.Dp * sizeof(float);
    l->xq = cv->take(rows); l->xv = cv->take(irows);
    l->key = cv->take(row); l->cw = cv->take(row); l->sq = cv->take(row);
    l->ib = cv->take(irow); l->io = cv->take(irow);
    l->pm = cv->take(row * p.nci); l->pe = cv->take(row * p.nci); l->psd = cv->take(row * p.nci);
    l->rmax = cv->take(row); l->cn = cv->take(row); l->dcoef = cv->take(row); l->rowloss = cv->take(row);
    l->off = host_off ? cv->take((size_t)NI * sizeof(float)) : 0;
    l->host_off = host_off;
    if (grads && query_side) { l->gpq = cv->take(rows * p.nci); l->gu = cv->take((size_t)B * gs * sizeof(float)); }
    if (grads && item_side) {
        l->gpv = cv->take(irows * p.ncs); l->bpart = cv->take(irow * p.ncs); l->npart = cv->take(irow * p.ncs);
        l->GV = cv->take((size_t)NI * D * sizeof(float)); l->Gb = cv->take((size_t)NI * sizeof(float));
    }
}

int orx_fullsoftmax_bind(orx_ctx* c, const FullSoftmaxLayout& l, const FullSoftmaxQuery& q, orx_table* V, orx_table* b, const float* item_offset,
                         int64_t B, float scale, float l2w, FullSoftmaxArgs* out) {
    FullSoftmaxArgs a;
    memset(&a, 0, sizeof(a));
    const FullSoftmaxPlan& p = l.plan;
    a.Q = q.Q; a.qid = q.qid; a.V = V->w; a.b = b ? b->w : nullptr;
    a.B = B; a.Bp = p.Bp; a.NQ = q.NQ; a.NI = V->rows; a.NIp = p.NIp;
    a.D = V->dim; a.Dp = (int)p.Dp; a.gs = (a.D + 1 + 3) & ~3;
    a.nci = (int)p.nci; a.tpi = (int)p.tpi; a.ncs = (int)p.ncs; a.tps = (int)p.tps;
    a.scale = scale; a.invB = 1.0f / (float)B; a.l2w = l2w; a.l2q = l2w; a.err = c->d_err;
    if (q.X0) { a.l2q = 0.f; a.X0 = q.X0; a.x0w = q.x0w; a.x0ld = q.x0ld; }          // the l2 term sits on x0, not on the query
    char* base = reinterpret_cast<char*>(c->d_tmp);
    auto f = [&](size_t o) { return reinterpret_cast<float*>(base + o); };
    a.xq = f(l.xq); a.xv = f(l.xv);
    a.key = reinterpret_cast<int32_t*>(base + l.key); a.cw = f(l.cw); a.sq = f(l.sq); a.ib = f(l.ib); a.io = f(l.io);
    a.pm = f(l.pm); a.pe = f(l.pe); a.psd = f(l.psd); a.rmax = f(l.rmax); a.cn = f(l.cn); a.dcoef = f(l.dcoef); a.rowloss = f(l.rowloss);
    a.gpq = f(l.gpq); a.gu = f(l.gu);
    a.gpv = f(l.gpv); a.bpart = f(l.bpart); a.npart = reinterpret_cast<int32_t*>(base + l.npart); a.GV = f(l.GV); a.Gb = f(l.Gb);
    a.off = item_offset;
    if (item_offset && l.host_off) {          // one float per ITEM: it lives where the ids live, and is not among the per-sample lists
        ORX_HIP(hipMemcpyAsync(f(l.off), item_offset, (size_t)a.NI * sizeof(float), hipMemcpyHostToDevice, c->stream));
        a.off = f(l.off);
    }
    *out = a;
    return ORX_OK;
}

int orx_fullsoftmax_mask(const char* fn, orx_table* b, int* train_mask) {
    const int every = ORX_TRAIN_USER | ORX_TRAIN_ITEM | ORX_TRAIN_BIAS;
    ORX_ARG((*train_mask & ~every) == 0, "%s: train mask 0x%x has bits outside ORX_TRAIN_USER | ORX_TRAIN_ITEM | ORX_TRAIN_BIAS", fn, *train_mask);
    ORX_ARG(b != nullptr || !(*train_mask & ORX_TRAIN_BIAS), "%s: ORX_TRAIN_BIAS without a bias table (bias is NULL)", fn);
    if (*train_mask == 0) *train_mask = ORX_TRAIN_USER | ORX_TRAIN_ITEM | (b ? ORX_TRAIN_BIAS : 0);
    return ORX_OK;
}

// ---- label sets (orx_seqrec_full_sets_step / orx_tower_sets_step and their forwards; kernels_labelsets.hip): what the two forms share
int orx_labelsets_check(const char* fn, const int32_t* lab_ptr, const int32_t* lab_items, int64_t B, int64_t n_lab, bool host) {
    ORX_ARG(n_lab >= 0 && n_lab < 0x80000000LL, "%s: n_lab = %lld (0 <= n_lab < 2^31)", fn, (long long)n_lab);
    if (B == 0) return ORX_OK;
    ORX_ARG(lab_ptr && (n_lab == 0 || lab_items), "%s: NULL label list", fn);
    if (!host) return ORX_OK;
    ORX_ARG(lab_ptr[0] == 0, "%s: lab_ptr[0] = %d, not 0", fn, lab_ptr[0]);
    for (int64_t i = 0; i < B; ++i)
        ORX_ARG(lab_ptr[i + 1] >= lab_ptr[i], "%s: lab_ptr decreases at sample %lld (%d after %d)", fn, (long long)i, lab_ptr[i + 1], lab_ptr[i]);
    ORX_ARG(lab_ptr[B] == n_lab, "%s: lab_ptr[B] = %d for n_lab = %lld label entries", fn, lab_ptr[B], (long long)n_lab);
    return ORX_OK;
}

void orx_labelsets_layout(Carve* cv, int64_t B, int32_t D, int64_t n_lab, bool host, bool host_tw, bool grads, LabelSetLayout* l) {
    memset(l, 0, sizeof(*l));
    if (host) { l->ptr = cv->take((size_t)(B + 1) * sizeof(int32_t)); l->items = cv->take((size_t)n_lab * sizeof(int32_t)); }
    if (host_tw) l->tw = cv->take((size_t)n_lab * sizeof(float));
    if (grads) { l->owner = cv->take((size_t)n_lab * sizeof(int32_t)); l->lp = cv->take((size_t)B * D * sizeof(float)); }
}

int orx_labelsets_bind(orx_ctx* c, const LabelSetLayout& l, const FullSoftmaxArgs& fs, const int32_t* lab_ptr, const int32_t* lab_items,
                       const float* lab_weight, int64_t n_lab, bool host, bool grads, LabelSetArgs* out) {
    LabelSetArgs a;
    memset(&a, 0, sizeof(a));
    char* base = reinterpret_cast<char*>(c->d_tmp);
    a.fs = fs; a.n = n_lab;
    BagArgs lists;                              // the label lists are staged as the bag lists are
    memset(&lists, 0, sizeof(lists));
    CHECK(orx_bag_stage(c, lab_ptr, lab_items, fs.B, n_lab, host, reinterpret_cast<int32_t*>(base + l.ptr), reinterpret_cast<int32_t*>(base + l.items), &lists));
    a.ptr = lists.ptr; a.items = lists.items;
    a.tw = lab_weight;
    if (lab_weight && host && n_lab) {          // one float per ENTRY: it lives where the ids live
        ORX_HIP(hipMemcpyAsync(base + l.tw, lab_weight, (size_t)n_lab * sizeof(float), hipMemcpyHostToDevice, c->stream));
        a.tw = reinterpret_cast<float*>(base + l.tw);
    }
    if (grads) { a.owner = reinterpret_cast<int32_t*>(base + l.owner); a.lp = reinterpret_cast<float*>(base + l.lp); }
    *out = a;
    return ORX_OK;
}

extern "C" int orx_fullsoftmax_geometry(int64_t B, int64_t NI, int32_t D, int32_t chunk_items, int32_t chunk_samples, int64_t out[6]) {
    static const char* fn = "orx_fullsoftmax_geometry";
    ORX_ARG(out, "%s: NULL out", fn);
    CHECK(orx_fullsoftmax_check(fn, B, NI, D, 1.0f, chunk_items, chunk_samples));
    Carve cv;
    FullSoftmaxLayout l;
    orx_fullsoftmax_layout(&cv, B, NI, D, chunk_items, chunk_samples, true, true, true, false, &l);
    out[0] = 64; out[1] = 64; out[2] = l.plan.nci; out[3] = l.plan.ncs; out[4] = l.plan.Dp; out[5] = (int64_t)cv.off;
    return ORX_OK;
}

// ---- the drivers
namespace {

// what a step and a forward share once their checks have passed: the NULL-id refusal, the lists on the device, the scratch of the
// form, of the full softmax and of the label sets in d_tmp, and the kernels' arguments (partial is the caller's to set per call)
int prepare(orx_ctx* c, FullSoftmaxForm& f, orx_table* V, orx_table* b, const int32_t* pid, const LabelLists* sets, const float* weight,
            const float* item_offset, int64_t B, float scale, float l2w, int32_t chunk_items, int32_t chunk_samples, bool grads, bool item_side, int flags,
            FullSoftmaxArgs* a, LabelSetArgs* ls) {
    ORX_ARG((sets || pid) && (!f.has_ids || f.ids), "%s: NULL id pointer", f.fn);
    ORX_HIP(hipSetDevice(c->device));
    const bool host = !(flags & ORX_IDS_DEVICE);
    StepInputs in;
    if (f.has_ids) CHECK(orx_stage_steps(c, 1, B, B, flags, {{f.ids, 1}, {pid, 1}}, {{weight, 1}}, &in));
    else CHECK(orx_stage_steps(c, 1, B, B, flags, {{pid, 1}}, {{weight, 1}}, &in));
    Carve cv;
    f.carve(&cv, grads);
    FullSoftmaxLayout lay;
    orx_fullsoftmax_layout(&cv, B, V->rows, V->dim, chunk_items, chunk_samples, grads, grads && f.query_side, item_side, host && item_offset, &lay);
    LabelSetLayout llay;
    if (sets) orx_labelsets_layout(&cv, B, V->dim, sets->n, host, host && sets->weight, grads, &llay);
    ENSURE(c->d_tmp, c->d_tmp_cap, cv.off);
    FullSoftmaxQuery q;
    memset(&q, 0, sizeof(q));
    q.qid = f.has_ids ? in.id[0] : nullptr;
    CHECK(f.bind(grads, &q));
    CHECK(orx_fullsoftmax_bind(c, lay, q, V, b, item_offset, B, scale, l2w, a));
    a->pid = in.id[f.has_ids ? 1 : 0]; a->wt = in.f[0];
    if (sets) CHECK(orx_labelsets_bind(c, llay, *a, sets->ptr, sets->items, sets->weight, sets->n, host, grads, ls));
    return ORX_OK;
}

}  // namespace

int orx_fullsoftmax_drive_step(orx_ctx* c, orx_opt* opt, FullSoftmaxForm& f, orx_table* V, orx_table* b, const int32_t* pid, const LabelLists* sets,
                               const float* weight, const float* item_offset, int64_t B, float scale, float l2_reg, int32_t chunk_items,
                               int32_t chunk_samples, int train_mask, int flags, float* loss_out, float* l2_out) {
    const char* fn = f.fn;
    CHECK(f.check());
    CHECK(orx_fullsoftmax_check(fn, B, V->rows, V->dim, scale, chunk_items, chunk_samples));
    CHECK(f.train(&train_mask));
    for (int i = 0; i < f.n_tab; ++i)
        if (!f.tab[i].dense) CHECK(orx_check_apply_rows_opt(opt, f.tab[i].t, nullptr));
    const bool host = !(flags & ORX_IDS_DEVICE);
    if (sets) CHECK(orx_labelsets_check(fn, sets->ptr, sets->items, B, sets->n, host));
    if (B == 0) return ORX_OK;
    const bool tV = (train_mask & ORX_TRAIN_ITEM) != 0, tb = (train_mask & ORX_TRAIN_BIAS) != 0;
    FullSoftmaxArgs a;
    LabelSetArgs ls;
    CHECK(prepare(c, f, V, b, pid, sets, weight, item_offset, B, scale, l2_reg, chunk_items, chunk_samples, true, tV || tb, flags, &a, &ls));
    // One rule for every table: V, b and the form's dense tables are read in full -- every row current, out of the lazy set; a table
    // outside the mask is finished under the old counter (whatever optimizer it is lazy under), then only read
    orx_table* keep[2 + sizeof(f.tab) / sizeof(f.tab[0])]; int n_keep = 0;
    for (int i = 0; i < f.n_tab; ++i)
        if (!f.tab[i].dense) { if (f.tab[i].trained) keep[n_keep++] = f.tab[i].t; else CHECK(orx_table_sync(f.tab[i].t)); }
    CHECK(orx_table_sync(V)); CHECK(orx_table_sync(b));
    if (tV) keep[n_keep++] = V;
    if (b && tb) keep[n_keep++] = b;
    for (int i = 0; i < f.n_tab; ++i)
        if (f.tab[i].dense) { CHECK(orx_table_sync(f.tab[i].t)); if (f.tab[i].t && f.tab[i].trained) keep[n_keep++] = f.tab[i].t; }

    const int rc = orx_run_steps(c, 1, orx_fullsoftmax_npartials(B), flags, loss_out, l2_out, nullptr, [&](int64_t, int64_t, float* partial) -> int {
        a.partial = partial;
        CHECK(f.produce(a, true));
        if (sets) {                         // (after the form has taken its pairs: the label entries are sorted by item on the same buffers)
            ls.fs = a;
            CHECK(orx_launch_labelsets_forward(c, ls));
            CHECK(orx_launch_labelsets_grads(c, ls, f.query_side, tV || tb));
        } else {
            CHECK(orx_launch_fullsoftmax_forward(c, a));
            CHECK(orx_launch_fullsoftmax_grads(c, a, f.query_side, tV || tb));
        }
        if (f.backward) CHECK(f.backward());
        if (opt->kind == ORX_ADAM) CHECK(orx_opt_advance(opt, keep, n_keep));      // once per step: after the step's reads, before its applies
        CHECK(f.apply(a));
        if (tV) CHECK(orx_table_apply_dense_at(c, opt, V, a.GV));
        if (tb) CHECK(orx_table_apply_dense_at(c, opt, b, a.Gb));
        return ORX_OK;
    });
    CHECK(rc);
    // device lists whose caller took the losses: the call has synchronised, so the index flag is looked at here as well
    if (f.index_flag && !host && (loss_out || l2_out)) return orx_check_index_error(c);
    return ORX_OK;
}

int orx_fullsoftmax_drive_loss(orx_ctx* c, FullSoftmaxForm& f, orx_table* V, orx_table* b, const int32_t* pid, const LabelLists* sets,
                               const float* weight, const float* item_offset, int64_t B, float scale, int32_t chunk_items, int flags,
                               float* loss_out, float* l2_out, float* row_loss_out) {
    const char* fn = f.fn;
    CHECK(f.check());
    CHECK(orx_fullsoftmax_check(fn, B, V->rows, V->dim, scale, chunk_items, 0));
    const bool host = !(flags & ORX_IDS_DEVICE);
    if (sets) CHECK(orx_labelsets_check(fn, sets->ptr, sets->items, B, sets->n, host));
    if (B == 0) {
        if (loss_out) *loss_out = 0.f;
        if (l2_out) *l2_out = 0.f;
        return ORX_OK;
    }
    FullSoftmaxArgs a;
    LabelSetArgs ls;
    CHECK(prepare(c, f, V, b, pid, sets, weight, item_offset, B, scale, 0.f, chunk_items, 0, false, false, flags, &a, &ls));
    return orx_run_forward(c, orx_fullsoftmax_npartials(B), loss_out, l2_out, [&](float* partial) -> int {
        a.partial = partial;
        CHECK(orx_table_sync(V)); CHECK(orx_table_sync(b));         // what is read in full: every row current
        for (int i = 0; i < f.n_tab; ++i)
            if (f.tab[i].dense) CHECK(orx_table_sync(f.tab[i].t));
        CHECK(f.produce(a, false));
        if (sets) { ls.fs = a; CHECK(orx_launch_labelsets_forward(c, ls)); }
        else CHECK(orx_launch_fullsoftmax_forward(c, a));
        if (row_loss_out)
            ORX_HIP(hipMemcpyAsync(row_loss_out, a.rowloss, (size_t)B * sizeof(float), host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
        return ORX_OK;
    });
}

// ---- the user-table form: Q is the user table itself, qid the staged uid
namespace {

// is_step: the step's checks (opt among them); otherwise the forward's
void user_form(FullSoftmaxForm* f, const char* fn, bool is_step, orx_ctx* c, orx_opt* opt, orx_table* U, orx_table* V, orx_table* b, const int32_t* uid,
               int64_t B, float l2_reg, int flags) {
    f->fn = fn; f->has_ids = true; f->ids = uid; f->index_flag = false; f->query_side = false;
    f->n_tab = 1; f->tab[0] = {U, false, false};
    f->check = [=]() -> int {
        if (is_step) return orx_check_dot_step(fn, c, opt, U, V, b, 0, 1, B, B, l2_reg, flags, FS_FLAGS);
        CHECK(orx_check_dot_model(fn, c, U, V, b, 0, flags, FS_FLAGS));
        ORX_ARG(!(flags & ORX_NO_L2), "%s: ORX_NO_L2 belongs to the step (the forward has no objective)", fn);
        return ORX_OK;
    };
    f->train = [=](int* mask) -> int {
        CHECK(orx_fullsoftmax_mask(fn, b, mask));
        f->tab[0].trained = f->query_side = (*mask & ORX_TRAIN_USER) != 0;
        return ORX_OK;
    };
    f->carve = [](Carve*, bool) {};
    f->bind = [=](bool, FullSoftmaxQuery* q) -> int { q->Q = U->w; q->NQ = U->rows; return ORX_OK; };
    f->produce = [=](const FullSoftmaxArgs& a, bool) -> int { return orx_table_touch(U, a.qid, B); };
    f->apply = [=](const FullSoftmaxArgs& a) -> int { return f->query_side ? orx_apply_rows(c, opt, U, nullptr, a.qid, B, a.gu, a.gs) : ORX_OK; };
}

}  // namespace

extern "C" int orx_fullsoftmax_step(orx_ctx* c, orx_opt* opt, orx_table* U, orx_table* V, orx_table* b,
                                    const int32_t* uid, const int32_t* pid, const float* weight, const float* item_offset,
                                    int64_t B, float scale, float l2_reg, int32_t chunk_items, int32_t chunk_samples, int train_mask, int flags,
                                    float* loss_out, float* l2_out) {
    FullSoftmaxForm f;
    user_form(&f, "orx_fullsoftmax_step", true, c, opt, U, V, b, uid, B, l2_reg, flags);
    return orx_fullsoftmax_drive_step(c, opt, f, V, b, pid, nullptr, weight, item_offset, B, scale, l2_reg, chunk_items, chunk_samples, train_mask, flags,
                                      loss_out, l2_out);
}

extern "C" int orx_fullsoftmax_loss(orx_ctx* c, orx_table* U, orx_table* V, orx_table* b,
                                    const int32_t* uid, const int32_t* pid, const float* weight, const float* item_offset,
                                    int64_t B, float scale, int32_t chunk_items, int flags, float* loss_out, float* l2_out, float* row_loss_out) {
    FullSoftmaxForm f;
    user_form(&f, "orx_fullsoftmax_loss", false, c, nullptr, U, V, b, uid, B, 0.f, flags);
    return orx_fullsoftmax_drive_loss(c, f, V, b, pid, nullptr, weight, item_offset, B, scale, chunk_items, flags, loss_out, l2_out, row_loss_out);
}
