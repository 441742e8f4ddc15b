// C-ABI entry points of the history-pooled recommender with a dense tower: orx_tower_step, orx_tower_loss, orx_tower_query and
// orx_tower_geometry (include/openrec_hip.h has the semantics, kernels_tower.hip the kernels), and orx_tower_sets_step /
// orx_tower_sets_loss, the step and the forward with a label set per sample (kernels_labelsets.hip).
//
// The step is orx_seqrec_full_step with the tower between the pool and the query.  Per step: everything is checked; the lists are
// staged; the lazy rows of every side table are touched with its id list, then bag_items is sorted and the lazy history rows are
// touched on the sorted list; the item table, the bias and every layer are read in full -- finished first, out of the lazy set;
// tower_input writes x0, uid', c_i and the owners; the sorted pairs' positions are replaced by their owners; one forward
// launch per layer; the full softmax's forward and gradient passes with Q = x_L (its query-side l2 coefficient 0, its l2 term taken
// on the rows of x0); one backward launch per layer, last to first; one finishing launch; [Adam: the counter advances]; then the
// applies: the pooled columns of g_0 scaled by c_i in place and orx_apply_rows_sorted of the history table, column slice j of g_0
// with f_j to orx_apply_rows of S_j -- both read g_0 where it lies, by its stride --, and the dense rule on V, b and every W_l, c_l.
// No kernel before the applies writes a table.  Scratch is carved from the context's grow-only d_tmp: O(B sum of widths) floats
// and the partials of the layers beyond what orx_seqrec_full_step takes.
#include <cmath>
#include <cstring>

#include "orx_graph.h"
#include "orx_internal.h"

namespace {

constexpr int TW_FLAGS = ORX_IDS_DEVICE | ORX_NO_L2 | ORX_HOGWILD | ORX_CENSOR;      // (the last two are named to be refused by name)

struct TowerModel {
    orx_table* hist; orx_table* item; orx_table* b;
    int m; orx_table* S[ORX_TOWER_SIDE]; const int32_t* f[ORX_TOWER_SIDE];
    int L; orx_table* W[ORX_TOWER_LAYERS]; orx_table* c[ORX_TOWER_LAYERS];
    int relu_last; int so; int w[ORX_TOWER_LAYERS + 1];
};

// out_dim: the width the last layer must have (the item table's dim, or the output table's)
int check_tower(const char* fn, orx_ctx* c, orx_table* hist, int32_t n_side, orx_table* const* side, const int32_t* const* side_ids,
                int32_t n_layers, orx_table* const* W, orx_table* const* cs, int relu_last, int out_dim, const char* out_name,
                std::initializer_list<orx_table*> others, int64_t B, TowerModel* md) {
    memset(md, 0, sizeof(*md));
    ORX_ARG(c && hist, "%s: NULL context/table", fn);
    ORX_ARG(n_layers >= 1 && n_layers <= ORX_TOWER_LAYERS, "%s: %d layers (1 .. %d)", fn, n_layers, ORX_TOWER_LAYERS);
    ORX_ARG(n_side >= 0 && n_side <= ORX_TOWER_SIDE, "%s: %d side tables (0 .. %d)", fn, n_side, ORX_TOWER_SIDE);
    ORX_ARG(W && (n_side == 0 || (side && (B == 0 || side_ids))), "%s: NULL table list", fn);
    md->hist = hist; md->m = n_side; md->L = n_layers; md->relu_last = relu_last != 0;
    // the tables: none NULL, none passed twice, all on the call's context -- then the widths
    std::vector<orx_table*> all(others);
    all.push_back(hist);
    for (int j = 0; j < n_side; ++j) {
        ORX_ARG(side[j] && (B == 0 || side_ids[j]), "%s: side table %d or its id list is NULL", fn, j);
        md->S[j] = side[j]; md->f[j] = B ? side_ids[j] : nullptr;
        all.push_back(side[j]);
    }
    for (int l = 0; l < n_layers; ++l) {
        ORX_ARG(W[l], "%s: layer %d is NULL", fn, l);
        md->W[l] = W[l]; md->c[l] = cs ? cs[l] : nullptr;
        all.push_back(W[l]);
        if (md->c[l]) all.push_back(md->c[l]);
    }
    for (size_t i = 0; i < all.size(); ++i) {
        if (!all[i]) continue;
        ORX_ARG(all[i]->ctx == c, "%s: the tables belong to a different context", fn);
        for (size_t k = 0; k < i; ++k)
            ORX_ARG(all[k] != all[i] && (!all[k] || all[k]->w != all[i]->w), "%s: a table is passed twice (tied tables are not offered)", fn);
    }
    int in0 = 0;
    for (int j = 0; j < n_side; ++j) {
        ORX_ARG(side[j]->dim >= 1 && side[j]->dim <= ORX_TOWER_WIDTH, "%s: side table %d has dim %d (1 .. %d)", fn, j, side[j]->dim, ORX_TOWER_WIDTH);
        in0 += side[j]->dim;
    }
    md->so = in0;
    ORX_ARG(hist->dim >= 1 && hist->dim <= ORX_TOWER_WIDTH, "%s: history dim %d outside [1, %d]", fn, hist->dim, ORX_TOWER_WIDTH);
    in0 += hist->dim;
    ORX_ARG(in0 <= ORX_TOWER_WIDTH, "%s: input width %d (the side dims and the history dim) above %d", fn, in0, ORX_TOWER_WIDTH);
    md->w[0] = in0;
    for (int l = 0; l < n_layers; ++l) {
        ORX_ARG(W[l]->dim >= 1 && W[l]->dim <= ORX_TOWER_WIDTH && W[l]->rows <= ORX_TOWER_WIDTH, "%s: layer %d is [%lld, %d]: a width outside [1, %d]", fn, l,
                (long long)W[l]->rows, W[l]->dim, ORX_TOWER_WIDTH);
        ORX_ARG(W[l]->rows == md->w[l], "%s: layer %d takes %lld inputs where %d arrive (the widths do not chain)", fn, l, (long long)W[l]->rows, md->w[l]);
        md->w[l + 1] = W[l]->dim;
        if (md->c[l])
            ORX_ARG(md->c[l]->rows == 1 && md->c[l]->dim == W[l]->dim, "%s: the bias of layer %d is [%lld, %d], not [1, %d]", fn, l,
                    (long long)md->c[l]->rows, md->c[l]->dim, W[l]->dim);
    }
    ORX_ARG(md->w[n_layers] == out_dim, "%s: the last layer is %d wide, %s has dim %d", fn, md->w[n_layers], out_name, out_dim);
    return ORX_OK;
}

int check_item(const char* fn, orx_table* hist, orx_table* item) {
    ORX_ARG(hist && item, "%s: NULL context/table", fn);
    ORX_ARG(hist->rows == item->rows, "%s: %lld history rows for %lld items", fn, (long long)hist->rows, (long long)item->rows);
    return ORX_OK;
}

struct TowerLayout {
    size_t uid, ptr, items, sid[ORX_TOWER_SIDE], coef, owner, pairs;
    size_t x[ORX_TOWER_LAYERS + 1], g[ORX_TOWER_LAYERS], pw[ORX_TOWER_LAYERS], pc[ORX_TOWER_LAYERS], GW[ORX_TOWER_LAYERS], Gc[ORX_TOWER_LAYERS];
    int ldx[ORX_TOWER_LAYERS + 1]; int nch, tpc;
};

// own_out: x_L is carved here (the step and the forward: the full softmax's Q); otherwise it is the caller's table
void tower_layout(Carve* cv, const int* w, int L, int m, int64_t B, int64_t n, bool host, bool own_out, bool lists, bool below, bool want_g0,
                  bool trained, TowerLayout* l) {
    memset(l, 0, sizeof(*l));
    orx_tower_plan(B, &l->nch, &l->tpc);
    l->uid = cv->take((size_t)B * sizeof(int32_t));
    if (host) {
        l->ptr = cv->take((size_t)(B + 1) * sizeof(int32_t)); l->items = cv->take((size_t)n * sizeof(int32_t));
        for (int j = 0; j < m; ++j) l->sid[j] = cv->take((size_t)B * sizeof(int32_t));
    }
    if (lists) { l->coef = cv->take((size_t)B * sizeof(float)); l->owner = cv->take((size_t)n * sizeof(int32_t)); l->pairs = cv->take((size_t)n * sizeof(uint2)); }
    for (int k = 0; k <= L; ++k) {
        l->ldx[k] = k < L ? (w[k] + 3) & ~3 : w[k];
        if (k < L || own_out) l->x[k] = cv->take((size_t)B * l->ldx[k] * sizeof(float));
    }
    for (int k = 0; k < L; ++k) {
        if (below && (k > 0 || want_g0)) l->g[k] = cv->take((size_t)B * l->ldx[k] * sizeof(float));
        if (trained) {
            const size_t kn = (size_t)w[k] * w[k + 1], nn = (size_t)w[k + 1];
            l->pw[k] = cv->take(kn * l->nch * sizeof(float)); l->pc[k] = cv->take(nn * l->nch * sizeof(float));
            l->GW[k] = cv->take(kn * sizeof(float)); l->Gc[k] = cv->take(nn * sizeof(float));
        }
    }
}

// the kernels' arguments on d_tmp once it is grown; host lists are copied here.  x[L] / g[L] are the caller's to set where not carved
int tower_bind(orx_ctx* c, const TowerModel& md, const TowerLayout& l, const int32_t* bag_ptr, const int32_t* bag_items, int64_t B, int64_t n,
               int mode, float denom, bool host, bool own_out, bool lists, bool below, bool want_g0, bool trained, TowerArgs* out) {
    TowerArgs t;
    memset(&t, 0, sizeof(t));
    char* base = reinterpret_cast<char*>(c->d_tmp);
    auto f = [&](size_t o) { return reinterpret_cast<float*>(base + o); };
    auto i32 = [&](size_t o) { return reinterpret_cast<int32_t*>(base + o); };
    t.L = md.L; t.m = md.m; t.relu_last = md.relu_last; t.so = md.so; t.B = B;
    t.nch = l.nch; t.tpc = l.tpc;
    for (int k = 0; k <= md.L; ++k) {
        t.w[k] = md.w[k]; t.ldx[k] = l.ldx[k]; t.ldg[k] = l.ldx[k];
        if (k < md.L || own_out) t.x[k] = f(l.x[k]);
    }
    for (int k = 0; k < md.L; ++k) {
        t.W[k] = md.W[k]->w; t.c[k] = md.c[k] ? md.c[k]->w : nullptr;
        if (below && (k > 0 || want_g0)) t.g[k] = f(l.g[k]);
        if (trained) { t.pw[k] = f(l.pw[k]); t.pc[k] = f(l.pc[k]); t.GW[k] = f(l.GW[k]); t.Gc[k] = f(l.Gc[k]); }
    }
    for (int j = 0; j < md.m; ++j) {
        t.S[j] = md.S[j]->w; t.srows[j] = md.S[j]->rows; t.sd[j] = md.S[j]->dim; t.f[j] = md.f[j];
        if (host) {
            ORX_HIP(hipMemcpyAsync(i32(l.sid[j]), md.f[j], (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            t.f[j] = i32(l.sid[j]);
        }
    }
    t.bag = orx_bag_args(c, md.hist, B, n, mode, denom);
    CHECK(orx_bag_stage(c, bag_ptr, bag_items, B, n, host, i32(l.ptr), i32(l.items), &t.bag));
    t.bag.uid = i32(l.uid);
    if (lists) { t.bag.coef = f(l.coef); t.bag.owner = i32(l.owner); }
    *out = t;
    return ORX_OK;
}

int touch_inputs(orx_ctx* c, const TowerModel& md, const TowerArgs& t, int64_t B, int64_t n, bool always, const uint2** sorted) {
    for (int j = 0; j < md.m; ++j) CHECK(orx_table_touch(md.S[j], t.f[j], B));
    return orx_bag_touch(c, md.hist, t.bag.items, n, always, sorted);       // (last: its pairs live until the context's next sort)
}

}  // namespace

extern "C" int orx_tower_geometry(int64_t B, int32_t n_layers, const int32_t* widths, int64_t out[4]) {
    static const char* fn = "orx_tower_geometry";
    ORX_ARG(out && widths, "%s: NULL argument", fn);
    ORX_ARG(n_layers >= 1 && n_layers <= ORX_TOWER_LAYERS, "%s: %d layers (1 .. %d)", fn, n_layers, ORX_TOWER_LAYERS);
    ORX_ARG(B >= 0 && B <= 0x7fffff00LL, "%s: B = %lld (B must fit 31 bits)", fn, (long long)B);
    int w[ORX_TOWER_LAYERS + 1];
    for (int k = 0; k <= n_layers; ++k) {
        ORX_ARG(widths[k] >= 1 && widths[k] <= ORX_TOWER_WIDTH, "%s: width %d outside [1, %d]", fn, widths[k], ORX_TOWER_WIDTH);
        w[k] = widths[k];
    }
    Carve cv;
    TowerLayout l;
    tower_layout(&cv, w, n_layers, 0, B, 0, false, true, true, true, true, true, &l);
    out[0] = 64; out[1] = l.nch; out[2] = l.tpc; out[3] = (int64_t)cv.off;
    return ORX_OK;
}

// the step with one label per sample (sets NULL) or a label set per sample (pid NULL)
static int tower_step(const char* fn, orx_ctx* c, orx_opt* opt, orx_table* hist, orx_table* item, orx_table* b,
                      int32_t n_side, orx_table* const* side, const int32_t* const* side_ids,
                      int32_t n_layers, orx_table* const* W, orx_table* const* cs, int relu_last,
                      const int32_t* bag_ptr, const int32_t* bag_items, const int32_t* pid, const LabelLists* sets, const float* weight,
                      const float* item_offset, int64_t B, int64_t n, int mode, float denom, float scale, float l2_reg, float l2_mlp,
                      int32_t chunk_items, int32_t chunk_samples, int train_mask, int flags, float* loss_out, float* l2_out) {
    CHECK(check_item(fn, hist, item));
    const bool host = !(flags & ORX_IDS_DEVICE);
    CHECK(orx_bag_check(fn, bag_ptr, bag_items, B, n, mode, denom, host));
    CHECK(orx_check_dot_step(fn, c, opt, item, item, b, 0, 1, B, B, l2_reg, flags, TW_FLAGS));
    ORX_ARG(std::isfinite(l2_mlp) && l2_mlp >= 0.f, "%s: l2_mlp must be finite and >= 0 (got %g)", fn, (double)l2_mlp);
    ORX_ARG(!(flags & ORX_NO_L2) || l2_mlp == 0.f, "%s: ORX_NO_L2 together with l2_mlp = %g (drop the flag, or pass l2_mlp = 0)", fn, (double)l2_mlp);
    TowerModel md;
    CHECK(check_tower(fn, c, hist, n_side, side, side_ids, n_layers, W, cs, relu_last, item->dim, "the item table", {item, b}, B, &md));
    md.item = item; md.b = b;
    CHECK(orx_fullsoftmax_check(fn, B, item->rows, item->dim, scale, chunk_items, chunk_samples));
    const int every = ORX_TRAIN_USER | ORX_TRAIN_ITEM | ORX_TRAIN_BIAS | ORX_TRAIN_SIDE | ORX_TRAIN_TOWER;
    ORX_ARG((train_mask & ~every) == 0, "%s: train mask 0x%x has bits outside ORX_TRAIN_USER | _ITEM | _BIAS | _SIDE | _TOWER", fn, train_mask);
    ORX_ARG(b != nullptr || !(train_mask & ORX_TRAIN_BIAS), "%s: ORX_TRAIN_BIAS without a bias table (bias is NULL)", fn);
    ORX_ARG(md.m > 0 || !(train_mask & ORX_TRAIN_SIDE), "%s: ORX_TRAIN_SIDE without a side table", fn);
    if (train_mask == 0) train_mask = ORX_TRAIN_USER | ORX_TRAIN_ITEM | (b ? ORX_TRAIN_BIAS : 0) | (md.m ? ORX_TRAIN_SIDE : 0) | ORX_TRAIN_TOWER;
    CHECK(orx_check_apply_rows_opt(opt, hist, nullptr));
    for (int j = 0; j < md.m; ++j) CHECK(orx_check_apply_rows_opt(opt, md.S[j], nullptr));
    if (sets) CHECK(orx_labelsets_check(fn, sets->ptr, sets->items, B, sets->n, host));
    if (B == 0) return ORX_OK;
    ORX_ARG(sets || pid, "%s: NULL id pointer", fn);
    ORX_HIP(hipSetDevice(c->device));
    const bool tH = (train_mask & ORX_TRAIN_USER) != 0, tV = (train_mask & ORX_TRAIN_ITEM) != 0, tb = (train_mask & ORX_TRAIN_BIAS) != 0;
    const bool tS = (train_mask & ORX_TRAIN_SIDE) != 0, tT = (train_mask & ORX_TRAIN_TOWER) != 0;
    const bool gH = tH && n > 0, want_g0 = gH || tS, below = want_g0 || tT;

    StepInputs in;
    CHECK(orx_stage_steps(c, 1, B, B, flags, {{pid, 1}}, {{weight, 1}}, &in));
    Carve cv;
    TowerLayout tl;
    tower_layout(&cv, md.w, md.L, md.m, B, n, host, true, true, below, want_g0, tT, &tl);
    FullSoftmaxLayout lay;
    orx_fullsoftmax_layout(&cv, B, item->rows, item->dim, chunk_items, chunk_samples, true, below, tV || tb, host && item_offset, &lay);
    LabelSetLayout llay;
    if (sets) orx_labelsets_layout(&cv, B, item->dim, sets->n, host, host && sets->weight, true, &llay);
    ENSURE(c->d_tmp, c->d_tmp_cap, cv.off);
    TowerArgs t;
    CHECK(tower_bind(c, md, tl, bag_ptr, bag_items, B, n, mode, denom, host, true, true, below, want_g0, tT, &t));
    t.l2x = l2_reg; t.l2m = l2_mlp;
    FullSoftmaxArgs a;
    CHECK(orx_fullsoftmax_bind(c, lay, t.x[md.L], B, item, b, item_offset, B, scale, l2_reg, &a));
    a.qid = t.bag.uid; a.pid = in.id[0]; a.wt = in.f[0];
    a.l2q = 0.f; a.X0 = t.x[0]; a.x0w = md.w[0]; a.x0ld = t.ldx[0];              // the l2 term sits on x0, not on the query
    t.g[md.L] = a.gu; t.ldg[md.L] = a.gs;
    LabelSetArgs ls;
    if (sets) CHECK(orx_labelsets_bind(c, llay, a, sets->ptr, sets->items, sets->weight, sets->n, host, true, &ls));
    uint2* pairs = reinterpret_cast<uint2*>(reinterpret_cast<char*>(c->d_tmp) + tl.pairs);
    // V, b and the layers are read in full: every row current, out of the lazy set; a table outside the mask is finished under the
    // old counter (whatever optimizer it is lazy under), then only read
    orx_table* keep[3 + ORX_TOWER_SIDE + 2 * ORX_TOWER_LAYERS]; int n_keep = 0;
    if (tH) keep[n_keep++] = hist; else CHECK(orx_table_sync(hist));
    for (int j = 0; j < md.m; ++j) { if (tS) keep[n_keep++] = md.S[j]; else CHECK(orx_table_sync(md.S[j])); }
    CHECK(orx_table_sync(item)); CHECK(orx_table_sync(b));
    if (tV) keep[n_keep++] = item;
    if (b && tb) keep[n_keep++] = b;
    for (int l = 0; l < md.L; ++l) {
        CHECK(orx_table_sync(md.W[l])); CHECK(orx_table_sync(md.c[l]));
        if (tT) { keep[n_keep++] = md.W[l]; if (md.c[l]) keep[n_keep++] = md.c[l]; }
    }

    const int rc = orx_run_steps(c, 1, orx_fullsoftmax_npartials(B), flags, loss_out, l2_out, nullptr, [&](int64_t, int64_t, float* partial) -> int {
        a.partial = partial;
        // ONE sort of bag_items serves the touch of the history rows and, its positions rewritten to their owners right after the
        // input launch (before anything else may sort), the apply -- as orx_seqrec_full_step has it
        const uint2* sorted = nullptr;
        CHECK(touch_inputs(c, md, t, B, n, tH, &sorted));
        CHECK(orx_launch_tower_input(c, t));
        if (sorted) CHECK(orx_launch_bag_owner_pairs(c, sorted, t.bag.owner, n, B, pairs));
        CHECK(orx_launch_tower_forward(c, t));
        if (sets) {                         // (after the pairs are taken: the label entries are sorted by item on the same buffers)
            ls.fs = a;
            CHECK(orx_launch_labelsets_forward(c, ls));
            CHECK(orx_launch_labelsets_grads(c, ls, below, tV || tb));
        } else {
            CHECK(orx_launch_fullsoftmax_forward(c, a));
            CHECK(orx_launch_fullsoftmax_grads(c, a, below, tV || tb));
        }
        if (below) CHECK(orx_launch_tower_backward(c, t));
        if (tT) CHECK(orx_launch_tower_finish(c, t));
        if (opt->kind == ORX_ADAM) CHECK(orx_opt_advance(opt, keep, n_keep));      // once per step: after the step's reads, before its applies
        if (gH) {
            CHECK(orx_launch_bag_scale_rows(c, t.g[0] + md.so, t.bag.coef, B, hist->dim, t.ldg[0]));
            CHECK(orx_apply_rows_sorted(c, opt, hist, pairs, n, t.g[0] + md.so, t.ldg[0]));
        }
        if (tS) {
            int c0 = 0;
            for (int j = 0; j < md.m; ++j) {
                CHECK(orx_apply_rows(c, opt, md.S[j], nullptr, t.f[j], B, t.g[0] + c0, t.ldg[0]));
                c0 += md.S[j]->dim;
            }
        }
        if (tT)
            for (int l = 0; l < md.L; ++l) {
                CHECK(orx_table_apply_dense_at(c, opt, md.W[l], t.GW[l]));
                if (md.c[l]) CHECK(orx_table_apply_dense_at(c, opt, md.c[l], t.Gc[l]));
            }
        return orx_fullsoftmax_apply_items(c, opt, item, b, tV, tb, a);
    });
    CHECK(rc);
    // device lists whose caller took the losses: the call has synchronised, so the index flag is looked at here as well
    if (!host && (loss_out || l2_out)) return orx_check_index_error(c);
    return ORX_OK;
}

static int tower_loss(const char* fn, orx_ctx* c, orx_table* hist, orx_table* item, orx_table* b,
                      int32_t n_side, orx_table* const* side, const int32_t* const* side_ids,
                      int32_t n_layers, orx_table* const* W, orx_table* const* cs, int relu_last,
                      const int32_t* bag_ptr, const int32_t* bag_items, const int32_t* pid, const LabelLists* sets, const float* weight,
                      const float* item_offset, int64_t B, int64_t n, int mode, float denom, float scale, int32_t chunk_items, int flags,
                      float* loss_out, float* l2_out, float* row_loss_out) {
    CHECK(check_item(fn, hist, item));
    const bool host = !(flags & ORX_IDS_DEVICE);
    CHECK(orx_bag_check(fn, bag_ptr, bag_items, B, n, mode, denom, host));
    CHECK(orx_check_dot_model(fn, c, item, item, b, 0, flags, ORX_IDS_DEVICE | ORX_HOGWILD | ORX_CENSOR));
    TowerModel md;
    CHECK(check_tower(fn, c, hist, n_side, side, side_ids, n_layers, W, cs, relu_last, item->dim, "the item table", {item, b}, B, &md));
    CHECK(orx_fullsoftmax_check(fn, B, item->rows, item->dim, scale, chunk_items, 0));
    if (sets) CHECK(orx_labelsets_check(fn, sets->ptr, sets->items, B, sets->n, host));
    if (B == 0) {
        if (loss_out) *loss_out = 0.f;
        if (l2_out) *l2_out = 0.f;
        return ORX_OK;
    }
    ORX_ARG(sets || pid, "%s: NULL id pointer", fn);
    ORX_HIP(hipSetDevice(c->device));
    StepInputs in;
    CHECK(orx_stage_steps(c, 1, B, B, flags, {{pid, 1}}, {{weight, 1}}, &in));
    Carve cv;
    TowerLayout tl;
    tower_layout(&cv, md.w, md.L, md.m, B, n, host, true, false, false, false, false, &tl);
    FullSoftmaxLayout lay;
    orx_fullsoftmax_layout(&cv, B, item->rows, item->dim, chunk_items, 0, false, false, false, host && item_offset, &lay);
    LabelSetLayout llay;
    if (sets) orx_labelsets_layout(&cv, B, item->dim, sets->n, host, host && sets->weight, false, &llay);
    ENSURE(c->d_tmp, c->d_tmp_cap, cv.off);
    TowerArgs t;
    CHECK(tower_bind(c, md, tl, bag_ptr, bag_items, B, n, mode, denom, host, true, false, false, false, false, &t));
    FullSoftmaxArgs a;
    CHECK(orx_fullsoftmax_bind(c, lay, t.x[md.L], B, item, b, item_offset, B, scale, 0.f, &a));
    a.qid = t.bag.uid; a.pid = in.id[0]; a.wt = in.f[0];
    a.l2q = 0.f; a.X0 = t.x[0]; a.x0w = md.w[0]; a.x0ld = t.ldx[0];
    LabelSetArgs ls;
    if (sets) CHECK(orx_labelsets_bind(c, llay, a, sets->ptr, sets->items, sets->weight, sets->n, host, false, &ls));
    return orx_run_forward(c, orx_fullsoftmax_npartials(B), loss_out, l2_out, [&](float* partial) -> int {
        a.partial = partial;
        CHECK(orx_table_sync(item)); CHECK(orx_table_sync(b));
        for (int l = 0; l < md.L; ++l) { CHECK(orx_table_sync(md.W[l])); CHECK(orx_table_sync(md.c[l])); }
        CHECK(touch_inputs(c, md, t, B, n, false, nullptr));
        CHECK(orx_launch_tower_input(c, t));
        CHECK(orx_launch_tower_forward(c, t));
        if (sets) { ls.fs = a; CHECK(orx_launch_labelsets_forward(c, ls)); }
        else CHECK(orx_launch_fullsoftmax_forward(c, a));
        if (row_loss_out)
            ORX_HIP(hipMemcpyAsync(row_loss_out, a.rowloss, (size_t)B * sizeof(float), host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
        return ORX_OK;
    });
}

extern "C" int orx_tower_step(orx_ctx* c, orx_opt* opt, orx_table* hist, orx_table* item, orx_table* b,
                              int32_t n_side, orx_table* const* side, const int32_t* const* side_ids,
                              int32_t n_layers, orx_table* const* W, orx_table* const* cs, int relu_last,
                              const int32_t* bag_ptr, const int32_t* bag_items, const int32_t* pid, const float* weight, const float* item_offset,
                              int64_t B, int64_t n, int mode, float denom, float scale, float l2_reg, float l2_mlp,
                              int32_t chunk_items, int32_t chunk_samples, int train_mask, int flags, float* loss_out, float* l2_out) {
    return tower_step("orx_tower_step", c, opt, hist, item, b, n_side, side, side_ids, n_layers, W, cs, relu_last, bag_ptr, bag_items, pid, nullptr,
                      weight, item_offset, B, n, mode, denom, scale, l2_reg, l2_mlp, chunk_items, chunk_samples, train_mask, flags, loss_out, l2_out);
}

extern "C" int orx_tower_loss(orx_ctx* c, orx_table* hist, orx_table* item, orx_table* b,
                              int32_t n_side, orx_table* const* side, const int32_t* const* side_ids,
                              int32_t n_layers, orx_table* const* W, orx_table* const* cs, int relu_last,
                              const int32_t* bag_ptr, const int32_t* bag_items, const int32_t* pid, const float* weight, const float* item_offset,
                              int64_t B, int64_t n, int mode, float denom, float scale, int32_t chunk_items, int flags,
                              float* loss_out, float* l2_out, float* row_loss_out) {
    return tower_loss("orx_tower_loss", c, hist, item, b, n_side, side, side_ids, n_layers, W, cs, relu_last, bag_ptr, bag_items, pid, nullptr, weight,
                      item_offset, B, n, mode, denom, scale, chunk_items, flags, loss_out, l2_out, row_loss_out);
}

// the same with a label set per sample (kernels_labelsets.hip)
extern "C" int orx_tower_sets_step(orx_ctx* c, orx_opt* opt, orx_table* hist, orx_table* item, orx_table* b,
                                   int32_t n_side, orx_table* const* side, const int32_t* const* side_ids,
                                   int32_t n_layers, orx_table* const* W, orx_table* const* cs, int relu_last,
                                   const int32_t* bag_ptr, const int32_t* bag_items,
                                   const int32_t* lab_ptr, const int32_t* lab_items, const float* lab_weight, int64_t n_lab,
                                   const float* weight, const float* item_offset,
                                   int64_t B, int64_t n, int mode, float denom, float scale, float l2_reg, float l2_mlp,
                                   int32_t chunk_items, int32_t chunk_samples, int train_mask, int flags, float* loss_out, float* l2_out) {
    const LabelLists sets{lab_ptr, lab_items, lab_weight, n_lab};
    return tower_step("orx_tower_sets_step", c, opt, hist, item, b, n_side, side, side_ids, n_layers, W, cs, relu_last, bag_ptr, bag_items, nullptr,
                      &sets, weight, item_offset, B, n, mode, denom, scale, l2_reg, l2_mlp, chunk_items, chunk_samples, train_mask, flags, loss_out,
                      l2_out);
}

extern "C" int orx_tower_sets_loss(orx_ctx* c, orx_table* hist, orx_table* item, orx_table* b,
                                   int32_t n_side, orx_table* const* side, const int32_t* const* side_ids,
                                   int32_t n_layers, orx_table* const* W, orx_table* const* cs, int relu_last,
                                   const int32_t* bag_ptr, const int32_t* bag_items,
                                   const int32_t* lab_ptr, const int32_t* lab_items, const float* lab_weight, int64_t n_lab,
                                   const float* weight, const float* item_offset,
                                   int64_t B, int64_t n, int mode, float denom, float scale, int32_t chunk_items, int flags,
                                   float* loss_out, float* l2_out, float* row_loss_out) {
    const LabelLists sets{lab_ptr, lab_items, lab_weight, n_lab};
    return tower_loss("orx_tower_sets_loss", c, hist, item, b, n_side, side, side_ids, n_layers, W, cs, relu_last, bag_ptr, bag_items, nullptr, &sets,
                      weight, item_offset, B, n, mode, denom, scale, chunk_items, flags, loss_out, l2_out, row_loss_out);
}

extern "C" int orx_tower_query(orx_ctx* c, orx_table* hist, int32_t n_side, orx_table* const* side, const int32_t* const* side_ids,
                               int32_t n_layers, orx_table* const* W, orx_table* const* cs, int relu_last,
                               const int32_t* bag_ptr, const int32_t* bag_items, int64_t B, int64_t n, int mode, float denom,
                               orx_table* out, int64_t out_row0, int flags) {
    static const char* fn = "orx_tower_query";
    ORX_ARG(c && hist && out, "%s: NULL context/table", fn);
    ORX_ARG((flags & ~ORX_IDS_DEVICE) == 0, "%s: flags other than ORX_IDS_DEVICE", fn);
    const bool host = !(flags & ORX_IDS_DEVICE);
    CHECK(orx_bag_check(fn, bag_ptr, bag_items, B, n, mode, denom, host));
    TowerModel md;
    CHECK(check_tower(fn, c, hist, n_side, side, side_ids, n_layers, W, cs, relu_last, out->dim, "the output table", {out}, B, &md));
    ORX_ARG(out_row0 >= 0 && out_row0 + B <= out->rows, "%s: rows [%lld, %lld) outside the %lld output rows", fn, (long long)out_row0,
            (long long)(out_row0 + B), (long long)out->rows);
    if (B == 0) return ORX_OK;
    ORX_HIP(hipSetDevice(c->device));
    CHECK(orx_table_sync(out));
    for (int l = 0; l < md.L; ++l) { CHECK(orx_table_sync(md.W[l])); CHECK(orx_table_sync(md.c[l])); }
    Carve cv;
    TowerLayout tl;
    tower_layout(&cv, md.w, md.L, md.m, B, n, host, false, false, false, false, false, &tl);
    ENSURE(c->d_tmp, c->d_tmp_cap, cv.off);
    TowerArgs t;
    CHECK(tower_bind(c, md, tl, bag_ptr, bag_items, B, n, mode, denom, host, false, false, false, false, false, &t));
    t.x[md.L] = out->w + (size_t)out_row0 * out->dim; t.ldx[md.L] = out->dim;
    CHECK(touch_inputs(c, md, t, B, n, false, nullptr));
    CHECK(orx_launch_tower_input(c, t));
    CHECK(orx_launch_tower_forward(c, t));
    out->version++;
    if (host) return orx_check_index_error(c);
    return ORX_OK;
}
