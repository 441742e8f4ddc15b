// C-ABI entry points of the history-pooled sequence recommender: orx_bag_pool, orx_seqrec_step and orx_seqrec_loss
// (include/openrec_hip.h has the semantics, kernels_bag.hip the kernels); what every call over bags shares -- the checks, the
// scratch layout and bind of the lists (BagLayout), the two halves of a step's history side (orx_bag_produce, orx_bag_apply);
// and at the end of the file the bag form of the softmax over all items: orx_seqrec_full_step / orx_seqrec_full_loss and, with
// a label set per sample, orx_seqrec_full_sets_step / orx_seqrec_full_sets_loss (the drivers are in api_fullsoftmax.hip).
//
// orx_seqrec_step is orx_multineg_step with the user row replaced by a pooled vector.  Per step: bag_items is sorted by row
// (orx_rows_sort) and the lazy history rows are touched on the sorted list; the pool writes Q [B][D] into scratch, an id list
// uid'[i] = i (-1: a dead bag), c_i and the owner of every list position; every sorted pair's position is replaced by its owner;
// pid and nid are touched as orx_multineg_step does; ONE gradient launch (orx_launch_multineg with U = Q, NU = B, uid = uid')
// writes per-occurrence gradient rows and pid | nid; [Adam: the counter advances]; g_q[i] is scaled by c_i in place and
// orx_apply_rows_sorted sums a history row's occurrences in list order out of the B rows of g_q -- the n x D occurrence rows
// never exist; then orx_apply_rows of the item table and the bias with pid | nid, as orx_multineg_step applies them.  No kernel
// before the applies writes a table, so every gradient is taken on the pre-step tables.  With a train mask that leaves the item
// table or the bias out, the two are applied as tables of their own on one sort of the list (as orx_vbpr_step does).  Scratch is
// carved from the context's grow-only d_tmp: O(n) words and O(B (1 + N) D).
#include <cmath>
#include <cstring>

#include "orx_internal.h"

namespace {

constexpr int SQ_FLAGS = ORX_IDS_DEVICE | ORX_NO_L2 | ORX_HOGWILD | ORX_CENSOR;      // (the last two are named to be refused by name)
constexpr int SQ_TRAIN_ALL = ORX_TRAIN_USER | ORX_TRAIN_ITEM | ORX_TRAIN_BIAS;

}  // namespace

// what the calls over bags (here and api_tower.hip) check of their lists before any device work; host lists are walked here
int orx_bag_check(const char* fn, const int32_t* bag_ptr, const int32_t* bag_items, int64_t B, int64_t n, int mode, float denom, bool host) {
    ORX_ARG(mode == ORX_BAG_MEAN || mode == ORX_BAG_FIXED, "%s: unknown pooling mode %d (ORX_BAG_MEAN, ORX_BAG_FIXED)", fn, mode);
    ORX_ARG(mode != ORX_BAG_FIXED || (std::isfinite(denom) && denom > 0.f), "%s: denom must be finite and > 0 (got %g)", fn, (double)denom);
    ORX_ARG(B >= 0 && B < 0x7fffffffLL, "%s: B = %lld (0 <= B < 2^31 - 1)", fn, (long long)B);
    ORX_ARG(n >= 0 && n < 0x80000000LL, "%s: n = %lld (0 <= n < 2^31)", fn, (long long)n);
    if (B == 0) return ORX_OK;
    ORX_ARG(bag_ptr && (n == 0 || bag_items), "%s: NULL bag list", fn);
    if (!host) return ORX_OK;
    ORX_ARG(bag_ptr[0] == 0, "%s: bag_ptr[0] = %d, not 0", fn, bag_ptr[0]);
    for (int64_t i = 0; i < B; ++i)
        ORX_ARG(bag_ptr[i + 1] >= bag_ptr[i], "%s: bag_ptr decreases at bag %lld (%d after %d)", fn, (long long)i, bag_ptr[i + 1], bag_ptr[i]);
    ORX_ARG(bag_ptr[B] == n, "%s: bag_ptr[B] = %d for n = %lld list entries", fn, bag_ptr[B], (long long)n);
    return ORX_OK;
}

static int check_model(const char* fn, orx_table* hist, orx_table* item) {
    ORX_ARG(hist && item, "%s: NULL context/table", fn);
    ORX_ARG(hist != item && hist->w != item->w, "%s: the history table and the item table are the same table (tied tables are not offered)", fn);
    ORX_ARG(hist->rows == item->rows, "%s: %lld history rows for %lld items", fn, (long long)hist->rows, (long long)item->rows);
    ORX_ARG(hist->dim <= 256, "%s: dim %d above 256", fn, hist->dim);
    return ORX_OK;
}

static int check_kind(const char* fn, int kind, int32_t N, int64_t B) {
    ORX_ARG(kind == ORX_MN_SOFTMAX || kind == ORX_MN_LOGSIG, "%s: unknown loss kind %d (ORX_MN_SOFTMAX, ORX_MN_LOGSIG)", fn, kind);
    ORX_ARG(N >= 1 && N <= 64, "%s: N must be in [1, 64], got %d", fn, N);
    ORX_ARG((B * (1 + (int64_t)N)) <= 0x7fffffffLL, "%s: B * (1 + N) must fit 31 bits", fn);
    return ORX_OK;
}

// the call's lists on the device: device lists pass through, host lists are copied into the two pieces of scratch
int orx_bag_stage(orx_ctx* c, const int32_t* bag_ptr, const int32_t* bag_items, int64_t B, int64_t n, bool host, int32_t* d_ptr, int32_t* d_items,
               BagArgs* a) {
    a->ptr = bag_ptr; a->items = bag_items;
    if (!host) return ORX_OK;
    ORX_HIP(hipMemcpyAsync(d_ptr, bag_ptr, (size_t)(B + 1) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (n) ORX_HIP(hipMemcpyAsync(d_items, bag_items, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    a->ptr = d_ptr; a->items = d_items;
    return ORX_OK;
}

void orx_bag_layout(Carve* cv, int64_t B, int64_t n, bool host, int keep, BagLayout* l) {
    memset(l, 0, sizeof(*l));
    l->keep = keep;
    if (keep >= ORX_BAG_FORWARD) l->uid = cv->take((size_t)B * sizeof(int32_t));
    if (host) { l->ptr = cv->take((size_t)(B + 1) * sizeof(int32_t)); l->items = cv->take((size_t)n * sizeof(int32_t)); }
    if (keep >= ORX_BAG_STEP) { l->coef = cv->take((size_t)B * sizeof(float)); l->owner = cv->take((size_t)n * sizeof(int32_t)); l->pairs = cv->take((size_t)n * sizeof(uint2)); }
}

int orx_bag_bind(orx_ctx* c, const BagLayout& l, orx_table* H, const int32_t* bag_ptr, const int32_t* bag_items, int64_t B, int64_t n, int mode,
                 float denom, bool host, BagArgs* out, uint2** pairs) {
    char* base = reinterpret_cast<char*>(c->d_tmp);
    auto i32 = [&](size_t o) { return reinterpret_cast<int32_t*>(base + o); };
    BagArgs a;
    memset(&a, 0, sizeof(a));
    a.H = H->w; a.rows = H->rows; a.D = H->dim; a.B = B; a.n = n; a.mode = mode;
    a.inv_denom = mode == ORX_BAG_FIXED ? 1.0f / denom : 0.f;
    a.err = c->d_err;
    CHECK(orx_bag_stage(c, bag_ptr, bag_items, B, n, host, i32(l.ptr), i32(l.items), &a));
    if (l.keep >= ORX_BAG_FORWARD) a.uid = i32(l.uid);
    if (l.keep >= ORX_BAG_STEP) { a.coef = reinterpret_cast<float*>(base + l.coef); a.owner = i32(l.owner); }
    if (pairs) *pairs = l.keep >= ORX_BAG_STEP ? reinterpret_cast<uint2*>(base + l.pairs) : nullptr;
    *out = a;
    return ORX_OK;
}

// The rows of H the bags read, brought up to date where H is lazily applied under Adam: on the sorted list -- a radix sort of the n
// ids and one launch -- and not by orx_table_touch, whose duplicate analysis takes 1 ms at n = 1.3M.  *sorted (may be NULL): the
// pairs, valid until the context's next sort, for a caller that applies with them; always sorted when `always`.
int orx_bag_touch(orx_ctx* c, orx_table* H, const int32_t* items, int64_t n, bool always, const uint2** sorted) {
    if (sorted) *sorted = nullptr;
    if (n == 0 || (!always && !H->lazy)) return ORX_OK;
    const uint2* s = nullptr;
    CHECK(orx_rows_sort(c, items, 1, n, n, H->rows, &s));
    if (sorted) *sorted = s;
    if (H->lazy) CHECK(orx_adam_rows_sorted(c, H->lazy, H, s, n, nullptr, 0, false));
    return ORX_OK;
}

// ONE sort of bag_items serves the touch of the history rows and, its positions rewritten to their owners right after the producing
// launch (before anything else may sort), the apply.  A history table outside the mask is current: no touch, no sort
int orx_bag_produce(orx_ctx* c, orx_table* H, const BagArgs& bag, uint2* pairs, const std::function<int()>& launch) {
    const uint2* sorted = nullptr;
    CHECK(orx_bag_touch(c, H, bag.items, bag.n, pairs != nullptr, pairs ? &sorted : nullptr));
    CHECK(launch());
    if (sorted) CHECK(orx_launch_bag_owner_pairs(c, sorted, bag.owner, bag.n, bag.B, pairs));
    return ORX_OK;
}

int orx_bag_apply(orx_ctx* c, orx_opt* opt, orx_table* H, const BagArgs& bag, const uint2* pairs, float* g, int col0, int ld) {
    CHECK(orx_launch_bag_scale_rows(c, g + col0, bag.coef, bag.B, bag.D, ld));
    return orx_apply_rows_sorted(c, opt, H, pairs, bag.n, g + col0, ld);
}

namespace {

// scratch of the step and of the forward (grads == false: the pooled rows and the lists alone)
struct Scratch { BagArgs bag; MultiNegArgs mn; uint2* pairs; uint2* isorted; };

int make_scratch(orx_ctx* c, orx_table* hist, orx_table* item, orx_table* b, const int32_t* bag_ptr, const int32_t* bag_items, int64_t B,
                 int64_t n, int32_t N, int mode, float denom, float l2w, bool host, bool grads, bool item_sorted, Scratch* out) {
    const int D = hist->dim, gs = (D + 1 + 3) & ~3;
    const int64_t nI = B * (1 + (int64_t)N);
    Carve cv;
    const size_t o_q = cv.take((size_t)B * D * sizeof(float));
    BagLayout bl;
    orx_bag_layout(&cv, B, n, host, grads ? ORX_BAG_STEP : ORX_BAG_FORWARD, &bl);
    size_t o_list = 0, o_gu = 0, o_gi = 0, o_isorted = 0;
    if (grads) {
        o_list = cv.take((size_t)nI * sizeof(int32_t)); o_gu = cv.take((size_t)B * gs * sizeof(float)); o_gi = cv.take((size_t)nI * gs * sizeof(float));
        if (item_sorted) o_isorted = cv.take((size_t)nI * sizeof(uint2));
    }
    ENSURE(c->d_tmp, c->d_tmp_cap, cv.off);
    char* base = reinterpret_cast<char*>(c->d_tmp);
    auto f = [&](size_t o) { return reinterpret_cast<float*>(base + o); };
    Scratch s;
    memset(&s, 0, sizeof(s));
    CHECK(orx_bag_bind(c, bl, hist, bag_ptr, bag_items, B, n, mode, denom, host, &s.bag, &s.pairs));
    s.bag.out = f(o_q);
    MultiNegArgs& a = s.mn;
    a.U = f(o_q); a.V = item->w; a.b = b ? b->w : nullptr; a.uid = s.bag.uid;
    a.B = B; a.NU = B; a.NI = item->rows; a.N = N; a.D = D; a.gs = gs;
    a.invB = 1.0f / (float)B; a.l2w = l2w; a.err = c->d_err;
    if (grads) {
        a.list = reinterpret_cast<int32_t*>(base + o_list); a.gu = f(o_gu); a.gi = f(o_gi);
        if (item_sorted) s.isorted = reinterpret_cast<uint2*>(base + o_isorted);
    }
    *out = s;
    return ORX_OK;
}

}  // namespace

extern "C" int orx_bag_pool(orx_ctx* c, orx_table* H, const int32_t* bag_ptr, const int32_t* bag_items, int64_t B, int64_t n, int mode,
                            float denom, orx_table* out, int64_t out_row0, int flags) {
    static const char* fn = "orx_bag_pool";
    ORX_ARG(c && H && out, "%s: NULL context/table", fn);
    ORX_ARG(H->ctx == c && out->ctx == c, "%s: the tables belong to a different context", fn);
    ORX_ARG((flags & ~ORX_IDS_DEVICE) == 0, "%s: flags other than ORX_IDS_DEVICE", fn);
    ORX_ARG(out != H && out->w != H->w, "%s: the output is the table that is pooled", fn);
    ORX_ARG(out->dim == H->dim, "%s: output dim %d != table dim %d", fn, out->dim, H->dim);
    ORX_ARG(H->dim <= 256, "%s: dim %d above 256", fn, H->dim);
    const bool host = !(flags & ORX_IDS_DEVICE);
    CHECK(orx_bag_check(fn, bag_ptr, bag_items, B, n, mode, denom, host));
    ORX_ARG(out_row0 >= 0 && out_row0 + B <= out->rows, "%s: rows [%lld, %lld) outside the %lld output rows", fn, (long long)out_row0,
            (long long)(out_row0 + B), (long long)out->rows);
    if (B == 0) return ORX_OK;
    ORX_HIP(hipSetDevice(c->device));
    CHECK(orx_table_sync(out));
    Carve cv;
    BagLayout bl;
    orx_bag_layout(&cv, B, n, host, ORX_BAG_STAGED, &bl);
    if (host) ENSURE(c->d_tmp, c->d_tmp_cap, cv.off);          // (device lists pass through: no scratch, and d_tmp is not touched)
    BagArgs a;
    CHECK(orx_bag_bind(c, bl, H, bag_ptr, bag_items, B, n, mode, denom, host, &a, nullptr));
    a.out = out->w + (size_t)out_row0 * out->dim;
    CHECK(orx_bag_touch(c, H, a.items, n, false, nullptr));
    CHECK(orx_launch_bag_pool(c, a));
    out->version++;
    if (host) return orx_check_index_error(c);
    return ORX_OK;
}

extern "C" int orx_seqrec_step(orx_ctx* c, int kind, orx_opt* opt, orx_table* hist, orx_table* item, orx_table* b,
                               const int32_t* bag_ptr, const int32_t* bag_items, const int32_t* pid, const int32_t* nid,
                               const float* weight, const float* neg_offset, int64_t B, int64_t n, int32_t N, int mode, float denom,
                               float l2_reg, int train_mask, int flags, float* loss_out, float* l2_out) {
    static const char* fn = "orx_seqrec_step";
    CHECK(check_model(fn, hist, item));
    const bool host = !(flags & ORX_IDS_DEVICE);
    CHECK(orx_bag_check(fn, bag_ptr, bag_items, B, n, mode, denom, host));
    CHECK(orx_check_dot_step(fn, c, opt, hist, item, b, 0, 1, B, B, l2_reg, flags, SQ_FLAGS));
    CHECK(check_kind(fn, kind, N, B));
    ORX_ARG((train_mask & ~SQ_TRAIN_ALL) == 0, "%s: train mask 0x%x has bits outside ORX_TRAIN_USER | ORX_TRAIN_ITEM | ORX_TRAIN_BIAS", fn, train_mask);
    ORX_ARG(b != nullptr || !(train_mask & ORX_TRAIN_BIAS), "%s: ORX_TRAIN_BIAS without a bias table (bias is NULL)", fn);
    const int all = ORX_TRAIN_USER | ORX_TRAIN_ITEM | (b ? ORX_TRAIN_BIAS : 0);
    if (train_mask == 0) train_mask = all;
    CHECK(orx_check_apply_rows_opt(opt, hist, nullptr));
    if (B == 0) return ORX_OK;
    ORX_ARG(pid && nid, "%s: NULL id pointer", fn);
    ORX_HIP(hipSetDevice(c->device));
    const bool tH = (train_mask & ORX_TRAIN_USER) != 0, tV = (train_mask & ORX_TRAIN_ITEM) != 0, tb = (train_mask & ORX_TRAIN_BIAS) != 0;
    const bool item_joint = tV && (tb || !b);           // the item table and the bias (if any) as orx_multineg_step applies them

    StepInputs in;
    CHECK(orx_stage_steps(c, 1, B, B, flags, {{pid, 1}, {nid, N}}, {{weight, 1}, {neg_offset, N}}, &in));
    Scratch s;
    CHECK(make_scratch(c, hist, item, b, bag_ptr, bag_items, B, n, N, mode, denom, l2_reg, host, true, !item_joint && (tV || tb), &s));
    MultiNegArgs& a = s.mn;
    a.pid = in.id[0]; a.nid = in.id[1]; a.wt = in.f[0]; a.off = in.f[1];
    const int gs = a.gs, D = a.D;
    const int64_t nI = B * (1 + (int64_t)N);
    // a table outside the mask is finished under the old counter (whatever optimizer it is lazy under), then only read
    orx_table* keep[3]; int n_keep = 0;
    if (tH) keep[n_keep++] = hist; else CHECK(orx_table_sync(hist));
    if (tV) keep[n_keep++] = item; else CHECK(orx_table_sync(item));
    if (b) { if (tb) keep[n_keep++] = b; else CHECK(orx_table_sync(b)); }

    const int rc = orx_run_steps(c, 1, orx_multineg_nwaves(c, D, B), flags, loss_out, l2_out, nullptr, [&](int64_t, int64_t, float* partial) -> int {
        a.partial = partial;
        CHECK(orx_bag_produce(c, hist, s.bag, tH ? s.pairs : nullptr, [&]() { return orx_launch_bag_pool(c, s.bag); }));
        CHECK(orx_touch_step(nullptr, item, b, nullptr, 0, a.pid, B, a.nid, B * N));
        CHECK(orx_launch_multineg(c, kind, true, a));
        if (opt->kind == ORX_ADAM) CHECK(orx_opt_advance(opt, keep, n_keep));      // once per step: after the step's reads, before its applies
        if (tH && n > 0) CHECK(orx_bag_apply(c, opt, hist, s.bag, s.pairs, a.gu, 0, gs));
        if (item_joint) return orx_apply_rows(c, opt, item, b, a.list, nI, a.gi, gs);
        if (tV || tb) {                     // one sort of pid | nid, each table on its own
            CHECK(orx_rows_sort_keep(c, a.list, 1, nI, nI, item->rows, s.isorted));
            if (tV) CHECK(orx_apply_rows_sorted(c, opt, item, s.isorted, nI, a.gi, gs));
            if (tb) CHECK(orx_apply_rows_sorted(c, opt, b, s.isorted, nI, a.gi + D, gs));
        }
        return ORX_OK;
    });
    CHECK(rc);
    // device lists whose caller took the losses: the call has synchronised, so the index flag is looked at here as well
    if (!host && (loss_out || l2_out)) return orx_check_index_error(c);
    return ORX_OK;
}

extern "C" int orx_seqrec_loss(orx_ctx* c, int kind, orx_table* hist, orx_table* item, orx_table* b,
                               const int32_t* bag_ptr, const int32_t* bag_items, const int32_t* pid, const int32_t* nid,
                               const float* weight, const float* neg_offset, int64_t B, int64_t n, int32_t N, int mode, float denom,
                               int flags, float* loss_out, float* l2_out) {
    static const char* fn = "orx_seqrec_loss";
    CHECK(check_model(fn, hist, item));
    const bool host = !(flags & ORX_IDS_DEVICE);
    CHECK(orx_bag_check(fn, bag_ptr, bag_items, B, n, mode, denom, host));
    CHECK(orx_check_dot_model(fn, c, hist, item, b, 0, flags, ORX_IDS_DEVICE | ORX_HOGWILD | ORX_CENSOR));
    CHECK(check_kind(fn, kind, N, B));
    if (B == 0) {
        if (loss_out) *loss_out = 0.f;
        if (l2_out) *l2_out = 0.f;
        return ORX_OK;
    }
    ORX_ARG(pid && nid, "%s: NULL id pointer", fn);
    ORX_HIP(hipSetDevice(c->device));
    StepInputs in;
    CHECK(orx_stage_steps(c, 1, B, B, flags, {{pid, 1}, {nid, N}}, {{weight, 1}, {neg_offset, N}}, &in));
    Scratch s;
    CHECK(make_scratch(c, hist, item, b, bag_ptr, bag_items, B, n, N, mode, denom, 0.f, host, false, false, &s));
    MultiNegArgs& a = s.mn;
    a.pid = in.id[0]; a.nid = in.id[1]; a.wt = in.f[0]; a.off = in.f[1];
    return orx_run_forward(c, orx_multineg_nwaves(c, a.D, B), loss_out, l2_out, [&](float* partial) -> int {
        a.partial = partial;
        CHECK(orx_bag_touch(c, hist, s.bag.items, n, false, nullptr));
        CHECK(orx_touch_step(nullptr, item, b, nullptr, 0, a.pid, B, a.nid, B * N));
        CHECK(orx_launch_bag_pool(c, s.bag));
        return orx_launch_multineg(c, kind, false, a);
    });
}

// ---- the softmax over ALL items with the pooled vector as the query: the bag form of api_fullsoftmax.hip's drivers.  The pool
// writes Q [B][D] and uid'[i] = i into scratch; the kernels take Q as their query table with NQ = B.  The history side is
// orx_seqrec_step's route
namespace {

struct BagForm : FullSoftmaxForm { BagLayout bl; size_t o_q; BagArgs bag; uint2* pairs; bool tH; };

// is_step: the step's checks (opt among them); otherwise the forward's
void bag_form(BagForm* f, const char* fn, bool is_step, orx_ctx* c, orx_opt* opt, orx_table* hist, orx_table* item, orx_table* b, const int32_t* bag_ptr,
              const int32_t* bag_items, int64_t B, int64_t n, int mode, float denom, float l2_reg, int flags) {
    const bool host = !(flags & ORX_IDS_DEVICE);
    f->fn = fn; f->has_ids = false; f->ids = nullptr; f->index_flag = true; f->query_side = f->tH = false;
    f->n_tab = 1; f->tab[0] = {hist, false, false};
    f->check = [=]() -> int {
        CHECK(check_model(fn, hist, item));
        CHECK(orx_bag_check(fn, bag_ptr, bag_items, B, n, mode, denom, host));
        if (is_step) return orx_check_dot_step(fn, c, opt, hist, item, b, 0, 1, B, B, l2_reg, flags, SQ_FLAGS);
        return orx_check_dot_model(fn, c, hist, item, b, 0, flags, ORX_IDS_DEVICE | ORX_HOGWILD | ORX_CENSOR);
    };
    f->train = [=](int* mask) -> int {
        CHECK(orx_fullsoftmax_mask(fn, b, mask));
        f->tab[0].trained = f->tH = (*mask & ORX_TRAIN_USER) != 0;
        f->query_side = f->tH && n > 0;
        return ORX_OK;
    };
    f->carve = [=](Carve* cv, bool grads) {
        f->o_q = cv->take((size_t)B * hist->dim * sizeof(float));
        orx_bag_layout(cv, B, n, host, grads ? ORX_BAG_STEP : ORX_BAG_FORWARD, &f->bl);
    };
    f->bind = [=](bool, FullSoftmaxQuery* q) -> int {
        CHECK(orx_bag_bind(c, f->bl, hist, bag_ptr, bag_items, B, n, mode, denom, host, &f->bag, &f->pairs));
        f->bag.out = reinterpret_cast<float*>(reinterpret_cast<char*>(c->d_tmp) + f->o_q);
        q->Q = f->bag.out; q->NQ = B; q->qid = f->bag.uid;
        return ORX_OK;
    };
    f->produce = [=](const FullSoftmaxArgs&, bool step) -> int {
        return orx_bag_produce(c, hist, f->bag, step && f->tH ? f->pairs : nullptr, [=]() { return orx_launch_bag_pool(c, f->bag); });
    };
    f->apply = [=](const FullSoftmaxArgs& a) -> int { return f->query_side ? orx_bag_apply(c, opt, hist, f->bag, f->pairs, a.gu, 0, a.gs) : ORX_OK; };
}

}  // namespace

extern "C" int orx_seqrec_full_step(orx_ctx* c, orx_opt* opt, orx_table* hist, orx_table* item, orx_table* b,
                                    const int32_t* bag_ptr, const int32_t* bag_items, const int32_t* pid, const float* weight,
                                    const float* item_offset, int64_t B, int64_t n, int mode, float denom, float scale, float l2_reg,
                                    int32_t chunk_items, int32_t chunk_samples, int train_mask, int flags, float* loss_out, float* l2_out) {
    BagForm f;
    bag_form(&f, "orx_seqrec_full_step", true, c, opt, hist, item, b, bag_ptr, bag_items, B, n, mode, denom, l2_reg, flags);
    return orx_fullsoftmax_drive_step(c, opt, f, item, b, pid, nullptr, weight, item_offset, B, scale, l2_reg, chunk_items, chunk_samples, train_mask,
                                      flags, loss_out, l2_out);
}

extern "C" int orx_seqrec_full_loss(orx_ctx* c, orx_table* hist, orx_table* item, orx_table* b,
                                    const int32_t* bag_ptr, const int32_t* bag_items, const int32_t* pid, const float* weight,
                                    const float* item_offset, int64_t B, int64_t n, int mode, float denom, float scale, int32_t chunk_items,
                                    int flags, float* loss_out, float* l2_out, float* row_loss_out) {
    BagForm f;
    bag_form(&f, "orx_seqrec_full_loss", false, c, nullptr, hist, item, b, bag_ptr, bag_items, B, n, mode, denom, 0.f, flags);
    return orx_fullsoftmax_drive_loss(c, f, item, b, pid, nullptr, weight, item_offset, B, scale, chunk_items, flags, loss_out, l2_out, row_loss_out);
}

// the same with a label set per sample (kernels_labelsets.hip)
extern "C" int orx_seqrec_full_sets_step(orx_ctx* c, orx_opt* opt, orx_table* hist, orx_table* item, orx_table* b,
                                         const int32_t* bag_ptr, const int32_t* bag_items,
                                         const int32_t* lab_ptr, const int32_t* lab_items, const float* lab_weight, int64_t n_lab,
                                         const float* weight, const float* item_offset, int64_t B, int64_t n, int mode, float denom, float scale,
                                         float l2_reg, int32_t chunk_items, int32_t chunk_samples, int train_mask, int flags,
                                         float* loss_out, float* l2_out) {
    const LabelLists sets{lab_ptr, lab_items, lab_weight, n_lab};
    BagForm f;
    bag_form(&f, "orx_seqrec_full_sets_step", true, c, opt, hist, item, b, bag_ptr, bag_items, B, n, mode, denom, l2_reg, flags);
    return orx_fullsoftmax_drive_step(c, opt, f, item, b, nullptr, &sets, weight, item_offset, B, scale, l2_reg, chunk_items, chunk_samples, train_mask,
                                      flags, loss_out, l2_out);
}

extern "C" int orx_seqrec_full_sets_loss(orx_ctx* c, orx_table* hist, orx_table* item, orx_table* b,
                                         const int32_t* bag_ptr, const int32_t* bag_items,
                                         const int32_t* lab_ptr, const int32_t* lab_items, const float* lab_weight, int64_t n_lab,
                                         const float* weight, const float* item_offset, int64_t B, int64_t n, int mode, float denom, float scale,
                                         int32_t chunk_items, int flags, float* loss_out, float* l2_out, float* row_loss_out) {
    const LabelLists sets{lab_ptr, lab_items, lab_weight, n_lab};
    BagForm f;
    bag_form(&f, "orx_seqrec_full_sets_loss", false, c, nullptr, hist, item, b, bag_ptr, bag_items, B, n, mode, denom, 0.f, flags);
    return orx_fullsoftmax_drive_loss(c, f, item, b, nullptr, &sets, weight, item_offset, B, scale, chunk_items, flags, loss_out, l2_out, row_loss_out);
}
