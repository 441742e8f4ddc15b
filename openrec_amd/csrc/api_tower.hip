// C-ABI entry points of the history-pooled recommender with a dense tower: orx_tower_step, orx_tower_loss, orx_tower_query and
// orx_tower_geometry (include/openrec_hip.h has the semantics, kernels_tower.hip the kernels), and orx_tower_sets_step /
// orx_tower_sets_loss, the step and the forward with a label set per sample.  The step and the forward are the tower form of the
// drivers in api_fullsoftmax.hip: this file holds what produces the query and what takes its gradient.
//
// Produce: the lazy rows of every side table are touched with its id list, then bag_items is sorted and the lazy history rows are
// touched on the sorted list; tower_input writes x0, uid', c_i and the owners; the sorted pairs' positions are replaced by their
// owners; one forward launch per layer.  The full softmax runs with Q = x_L (its query-side l2 coefficient 0, its l2 term taken
// on the rows of x0).  Backward: one launch per layer, last to first; one finishing launch.  Apply: the pooled columns of g_0
// scaled by c_i in place and orx_apply_rows_sorted of the history table, column slice j of g_0 with f_j to orx_apply_rows of S_j
// -- both read g_0 where it lies, by its stride --, and the dense rule on every W_l, c_l.  Scratch is carved from the context's
// grow-only d_tmp: O(B sum of widths) floats and the partials of the layers beyond what the bag form takes.
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
    BagLayout bag; size_t sid[ORX_TOWER_SIDE];
    size_t x[ORX_TOWER_LAYERS + 1], g[ORX_TOWER_LAYERS], pw[ORX_TOWER_LAYERS], pc[ORX_TOWER_LAYERS], GW[ORX_TOWER_LAYERS], Gc[ORX_TOWER_LAYERS];
    int ldx[ORX_TOWER_LAYERS + 1]; int nch, tpc;
};

// own_out: x_L is carved here (the step and the forward: the full softmax's Q); otherwise it is the caller's table
void tower_layout(Carve* cv, const int* w, int L, int m, int64_t B, int64_t n, bool host, bool own_out, bool lists, bool below, bool want_g0,
                  bool trained, TowerLayout* l) {
    memset(l, 0, sizeof(*l));
    orx_tower_plan(B, &l->nch, &l->tpc);
    orx_bag_layout(cv, B, n, host, lists ? ORX_BAG_STEP : ORX_BAG_FORWARD, &l->bag);
    if (host)
        for (int j = 0; j < m; ++j) l->sid[j] = cv->take((size_t)B * sizeof(int32_t));
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
               int mode, float denom, bool host, bool own_out, bool below, bool want_g0, bool trained, TowerArgs* out, uint2** pairs) {
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
    CHECK(orx_bag_bind(c, l.bag, md.hist, bag_ptr, bag_items, B, n, mode, denom, host, &t.bag, pairs));
    *out = t;
    return ORX_OK;
}

// the side rows, then the history rows on the sorted list (last: its pairs live until the context's next sort), x0, the owners
int tower_input(orx_ctx* c, const TowerModel& md, const TowerArgs& t, uint2* pairs) {
    for (int j = 0; j < md.m; ++j) CHECK(orx_table_touch(md.S[j], t.f[j], t.B));
    return orx_bag_produce(c, md.hist, t.bag, pairs, [&]() { return orx_launch_tower_input(c, t); });
}

// ---- the tower form of the full-softmax drivers: Q = x_L
struct TowerForm : FullSoftmaxForm {
    TowerModel md; TowerLayout tl; TowerArgs t; uint2* pairs;
    bool tH, tS, tT, gH, want_g0, below;
};

// is_step: the step's checks (opt among them); otherwise the forward's
void tower_form(TowerForm* f, const char* fn, bool is_step, orx_ctx* c, orx_opt* opt, orx_table* hist, orx_table* item, orx_table* b,
                int32_t n_side, orx_table* const* side, const int32_t* const* side_ids, int32_t n_layers, orx_table* const* W, orx_table* const* cs,
                int relu_last, const int32_t* bag_ptr, const int32_t* bag_items, int64_t B, int64_t n, int mode, float denom, float l2_reg,
                float l2_mlp, int flags) {
    const bool host = !(flags & ORX_IDS_DEVICE);
    f->fn = fn; f->has_ids = false; f->ids = nullptr; f->index_flag = true; f->n_tab = 0;
    f->query_side = f->tH = f->tS = f->tT = f->gH = f->want_g0 = f->below = false;
    f->check = [=]() -> int {
        CHECK(check_item(fn, hist, item));
        CHECK(orx_bag_check(fn, bag_ptr, bag_items, B, n, mode, denom, host));
        if (is_step) {
            CHECK(orx_check_dot_step(fn, c, opt, item, item, b, 0, 1, B, B, l2_reg, flags, TW_FLAGS));
            ORX_ARG(std::isfinite(l2_mlp) && l2_mlp >= 0.f, "%s: l2_mlp must be finite and >= 0 (got %g)", fn, (double)l2_mlp);
            ORX_ARG(!(flags & ORX_NO_L2) || l2_mlp == 0.f, "%s: ORX_NO_L2 together with l2_mlp = %g (drop the flag, or pass l2_mlp = 0)", fn, (double)l2_mlp);
        } else {
            CHECK(orx_check_dot_model(fn, c, item, item, b, 0, flags, ORX_IDS_DEVICE | ORX_HOGWILD | ORX_CENSOR));
        }
        TowerModel& md = f->md;
        CHECK(check_tower(fn, c, hist, n_side, side, side_ids, n_layers, W, cs, relu_last, item->dim, "the item table", {item, b}, B, &md));
        md.item = item; md.b = b;
        f->n_tab = 0;
        f->tab[f->n_tab++] = {hist, false, false};
        for (int j = 0; j < md.m; ++j) f->tab[f->n_tab++] = {md.S[j], false, false};
        for (int l = 0; l < md.L; ++l) { f->tab[f->n_tab++] = {md.W[l], true, false}; f->tab[f->n_tab++] = {md.c[l], true, false}; }
        return ORX_OK;
    };
    f->train = [=](int* mask) -> int {
        const TowerModel& md = f->md;
        const int every = ORX_TRAIN_USER | ORX_TRAIN_ITEM | ORX_TRAIN_BIAS | ORX_TRAIN_SIDE | ORX_TRAIN_TOWER;
        ORX_ARG((*mask & ~every) == 0, "%s: train mask 0x%x has bits outside ORX_TRAIN_USER | _ITEM | _BIAS | _SIDE | _TOWER", fn, *mask);
        ORX_ARG(b != nullptr || !(*mask & ORX_TRAIN_BIAS), "%s: ORX_TRAIN_BIAS without a bias table (bias is NULL)", fn);
        ORX_ARG(md.m > 0 || !(*mask & ORX_TRAIN_SIDE), "%s: ORX_TRAIN_SIDE without a side table", fn);
        if (*mask == 0) *mask = ORX_TRAIN_USER | ORX_TRAIN_ITEM | (b ? ORX_TRAIN_BIAS : 0) | (md.m ? ORX_TRAIN_SIDE : 0) | ORX_TRAIN_TOWER;
        f->tH = (*mask & ORX_TRAIN_USER) != 0; f->tS = (*mask & ORX_TRAIN_SIDE) != 0; f->tT = (*mask & ORX_TRAIN_TOWER) != 0;
        f->gH = f->tH && n > 0; f->want_g0 = f->gH || f->tS; f->below = f->want_g0 || f->tT;
        f->query_side = f->below;
        for (int i = 0; i < f->n_tab; ++i) f->tab[i].trained = i == 0 ? f->tH : f->tab[i].dense ? f->tT : f->tS;
        return ORX_OK;
    };
    f->carve = [=](Carve* cv, bool grads) {
        tower_layout(cv, f->md.w, f->md.L, f->md.m, B, n, host, true, grads, f->below, f->want_g0, f->tT, &f->tl);
    };
    f->bind = [=](bool, FullSoftmaxQuery* q) -> int {
        TowerArgs& t = f->t;
        CHECK(tower_bind(c, f->md, f->tl, bag_ptr, bag_items, B, n, mode, denom, host, true, f->below, f->want_g0, f->tT, &t, &f->pairs));
        t.l2x = l2_reg; t.l2m = l2_mlp;
        q->Q = t.x[f->md.L]; q->NQ = B; q->qid = t.bag.uid;
        q->X0 = t.x[0]; q->x0w = f->md.w[0]; q->x0ld = t.ldx[0];
        return ORX_OK;
    };
    f->produce = [=](const FullSoftmaxArgs& a, bool step) -> int {
        TowerArgs& t = f->t;
        if (step) { t.g[t.L] = a.gu; t.ldg[t.L] = a.gs; }             // the full softmax's query gradient is the last layer's
        CHECK(tower_input(c, f->md, t, step && f->tH ? f->pairs : nullptr));
        return orx_launch_tower_forward(c, t);
    };
    f->backward = [=]() -> int {
        if (f->below) CHECK(orx_launch_tower_backward(c, f->t));
        if (f->tT) CHECK(orx_launch_tower_finish(c, f->t));
        return ORX_OK;
    };
    f->apply = [=](const FullSoftmaxArgs&) -> int {
        const TowerModel& md = f->md;
        TowerArgs& t = f->t;
        if (f->gH) CHECK(orx_bag_apply(c, opt, hist, t.bag, f->pairs, t.g[0], md.so, t.ldg[0]));
        if (f->tS) {
            int c0 = 0;
            for (int j = 0; j < md.m; ++j) {
                CHECK(orx_apply_rows(c, opt, md.S[j], nullptr, t.f[j], B, t.g[0] + c0, t.ldg[0]));
                c0 += md.S[j]->dim;
            }
        }
        if (f->tT)
            for (int l = 0; l < md.L; ++l) {
                CHECK(orx_table_apply_dense_at(c, opt, md.W[l], t.GW[l]));
                if (md.c[l]) CHECK(orx_table_apply_dense_at(c, opt, md.c[l], t.Gc[l]));
            }
        return ORX_OK;
    };
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

extern "C" int orx_tower_step(orx_ctx* c, orx_opt* opt, orx_table* hist, orx_table* item, orx_table* b,
                              int32_t n_side, orx_table* const* side, const int32_t* const* side_ids,
                              int32_t n_layers, orx_table* const* W, orx_table* const* cs, int relu_last,
                              const int32_t* bag_ptr, const int32_t* bag_items, const int32_t* pid, const float* weight, const float* item_offset,
                              int64_t B, int64_t n, int mode, float denom, float scale, float l2_reg, float l2_mlp,
                              int32_t chunk_items, int32_t chunk_samples, int train_mask, int flags, float* loss_out, float* l2_out) {
    TowerForm f;
    tower_form(&f, "orx_tower_step", true, c, opt, hist, item, b, n_side, side, side_ids, n_layers, W, cs, relu_last, bag_ptr, bag_items, B, n, mode, denom,
               l2_reg, l2_mlp, flags);
    return orx_fullsoftmax_drive_step(c, opt, f, item, b, pid, nullptr, weight, item_offset, B, scale, l2_reg, chunk_items, chunk_samples, train_mask,
                                      flags, loss_out, l2_out);
}

extern "C" int orx_tower_loss(orx_ctx* c, orx_table* hist, orx_table* item, orx_table* b,
                              int32_t n_side, orx_table* const* side, const int32_t* const* side_ids,
                              int32_t n_layers, orx_table* const* W, orx_table* const* cs, int relu_last,
                              const int32_t* bag_ptr, const int32_t* bag_items, const int32_t* pid, const float* weight, const float* item_offset,
                              int64_t B, int64_t n, int mode, float denom, float scale, int32_t chunk_items, int flags,
                              float* loss_out, float* l2_out, float* row_loss_out) {
    TowerForm f;
    tower_form(&f, "orx_tower_loss", false, c, nullptr, hist, item, b, n_side, side, side_ids, n_layers, W, cs, relu_last, bag_ptr, bag_items, B, n, mode, denom,
               0.f, 0.f, flags);
    return orx_fullsoftmax_drive_loss(c, f, item, b, pid, nullptr, weight, item_offset, B, scale, chunk_items, flags, loss_out, l2_out, row_loss_out);
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
    TowerForm f;
    tower_form(&f, "orx_tower_sets_step", true, c, opt, hist, item, b, n_side, side, side_ids, n_layers, W, cs, relu_last, bag_ptr, bag_items, B, n, mode,
               denom, l2_reg, l2_mlp, flags);
    return orx_fullsoftmax_drive_step(c, opt, f, item, b, nullptr, &sets, weight, item_offset, B, scale, l2_reg, chunk_items, chunk_samples, train_mask,
                                      flags, loss_out, l2_out);
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
    TowerForm f;
    tower_form(&f, "orx_tower_sets_loss", false, c, nullptr, hist, item, b, n_side, side, side_ids, n_layers, W, cs, relu_last, bag_ptr, bag_items, B, n, mode,
               denom, 0.f, 0.f, flags);
    return orx_fullsoftmax_drive_loss(c, f, item, b, nullptr, &sets, weight, item_offset, B, scale, chunk_items, flags, loss_out, l2_out, row_loss_out);
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
    CHECK(tower_bind(c, md, tl, bag_ptr, bag_items, B, n, mode, denom, host, false, false, false, false, &t, nullptr));
    t.x[md.L] = out->w + (size_t)out_row0 * out->dim; t.ldx[md.L] = out->dim;
    CHECK(tower_input(c, md, t, nullptr));
    CHECK(orx_launch_tower_forward(c, t));
    out->version++;
    if (host) return orx_check_index_error(c);
    return ORX_OK;
}
