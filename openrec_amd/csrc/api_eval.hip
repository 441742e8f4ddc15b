// The host driver the read-only calls share -- scoring, top-K and the ranking metrics (orx_internal.h has the contracts): the table
// sync, the scorer's and the lists' argument checks, the staging of a batch's CSR lists and user ids, the scratch layout and the
// batch search, the one CSR metrics batch -- and the entry points that are little more than these parts: orx_score_all_items(_device),
// orx_rank_metrics, orx_rank_metrics_csr.  Host code only; api_topk.hip, api_evalmf.hip and api_cand.hip hold what is their route's own.
#include <algorithm>
#include <cstring>

#include "orx_internal.h"

// ---- argument checks, all on the host ---------------------------------------------------------------------------------
int orx_sync_tables(std::initializer_list<orx_table*> tables) {
    for (orx_table* t : tables) if (t) CHECK(orx_table_sync(t));
    return ORX_OK;
}

int orx_check_scorer(const char* fn, orx_ctx* c, int kind, orx_table* U, orx_table* V, orx_table* b, orx_table* w,
                     const int32_t* uid, int64_t n, bool check_uid_on_host) {
    ORX_ARG(kind >= 0 && kind <= 2, "%s: unknown kind %d", fn, kind);
    ORX_ARG(U->dim == V->dim && (!b || (b->rows == V->rows && b->dim == 1)), "%s: table shapes do not match", fn);
    ORX_ARG(kind != 2 || (w && w->rows == U->dim && w->dim == 1), "%s: GMF needs w [D, 1]", fn);
    ORX_ARG(U->dim <= 1024, "%s: dim too large for the LDS user tile", fn);
    for (int64_t q = 0; check_uid_on_host && q < n; ++q) {
        if (uid[q] < 0 || uid[q] >= U->rows) {
            orx_set_error("%s: user id %d outside [0, %lld)", fn, uid[q], (long long)U->rows);
            return ORX_ERR_INDEX;
        }
    }
    return ORX_OK;
}

int orx_check_lists(const char* fn, const char* what, const int64_t* ptr, const int32_t* items, int64_t n, int64_t NI,
                    bool ascending, int64_t* longest) {
    ORX_ARG(ptr[0] == 0, "%s: the %s lists start at offset 0", fn, what);
    int64_t m = 0;
    for (int64_t q = 0; q < n; ++q) {
        ORX_ARG(ptr[q + 1] >= ptr[q], "%s: %s offsets must not decrease", fn, what);
        m = std::max(m, ptr[q + 1] - ptr[q]);
    }
    if (longest) *longest = m;
    ORX_ARG(ptr[n] == 0 || items, "%s: NULL %s item list", fn, what);
    for (int64_t q = 0; q < n; ++q) {
        for (int64_t i = ptr[q]; i < ptr[q + 1]; ++i) {
            if (items[i] < 0 || items[i] >= NI) {
                orx_set_error("%s: %s id %d of user %lld outside [0, %lld)", fn, what, items[i], (long long)q, (long long)NI);
                return ORX_ERR_INDEX;
            }
            ORX_ARG(!ascending || i == ptr[q] || items[i] > items[i - 1],
                    "%s: the %s list of user %lld is not strictly ascending (item %d after %d)", fn, what, (long long)q, items[i],
                    i == ptr[q] ? 0 : items[i - 1]);
        }
    }
    return ORX_OK;
}

// ---- scratch layout and batch search ------------------------------------------------------------------------------------
size_t orx_layout(const size_t* sizes, int n, size_t* off) {
    Carve cv;
    for (int i = 0; i < n; ++i) off[i] = cv.take(sizes[i]);
    return cv.off;
}

int64_t orx_largest_batch(int64_t lo, int64_t hi, const std::function<bool(int64_t)>& fits) {
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) / 2;
        if (fits(mid)) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- staging of one batch ---------------------------------------------------------------------------------------------------
static CsrSlice csr_offsets(const int64_t* ptr, int64_t q0, int64_t nq, int64_t* hp) {
    CsrSlice s{ptr[q0], ptr[q0 + nq] - ptr[q0], 0};
    for (int64_t q = 0; q <= nq; ++q) hp[q] = ptr[q0 + q] - s.first;
    for (int64_t q = 0; q < nq; ++q) s.longest = std::max(s.longest, hp[q + 1] - hp[q]);
    return s;
}

CsrSlice orx_pack_csr(const int64_t* ptr, const int32_t* items, int64_t q0, int64_t nq, int64_t* hp, void* hi) {
    const CsrSlice s = csr_offsets(ptr, q0, nq, hp);
    if (s.count) memcpy(hi, items + s.first, 4 * (size_t)s.count);
    return s;
}

int orx_stage_csr(orx_ctx* c, const int64_t* ptr, const int32_t* items, int64_t q0, int64_t nq, int64_t* hp,
                  std::vector<int32_t>* sorted, int64_t* d_ptr, int32_t* d_items, CsrSlice* out) {
    const CsrSlice s = csr_offsets(ptr, q0, nq, hp);
    const int32_t* src = items + s.first;
    if (sorted) {
        sorted->assign(src, src + s.count);
        for (int64_t q = 0; q < nq; ++q)
            if (!std::is_sorted(sorted->begin() + hp[q], sorted->begin() + hp[q + 1])) std::sort(sorted->begin() + hp[q], sorted->begin() + hp[q + 1]);
        src = sorted->data();
    }
    ORX_HIP(hipMemcpyAsync(d_ptr, hp, (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (s.count) ORX_HIP(hipMemcpyAsync(d_items, src, (size_t)s.count * 4, hipMemcpyHostToDevice, c->stream));
    if (out) *out = s;
    return ORX_OK;
}

int orx_stage_uid_rows(orx_ctx* c, const int32_t* uid, int64_t nq, int64_t rows) {
    ENSURE(c->d_ids, c->d_ids_cap, (size_t)rows * sizeof(int32_t));
    if (rows == nq) return stage_ids(c, uid, nq, 0);
    static thread_local std::vector<int32_t> huid;
    huid.assign(uid, uid + nq);
    huid.resize(rows, uid[0]);                        // rows beyond the batch: the scorer's wide tile, their scores are never read
    return stage_ids(c, huid.data(), rows, 0);
}

int orx_evalbits_reserve(orx_ctx* c, size_t bytes) {
    if (bytes <= c->d_evalbits_cap) return ORX_OK;
    if (c->d_evalbits) ORX_HIP(hipFree(c->d_evalbits));
    c->d_evalbits = nullptr; c->d_evalbits_cap = 0;
    ORX_HIP(hipMalloc((void**)&c->d_evalbits, bytes));
    c->d_evalbits_cap = bytes;
    ORX_HIP(hipMemsetAsync(c->d_evalbits, 0, bytes, c->stream));
    return ORX_OK;
}

int orx_fetch_metrics(orx_ctx* c, const float* d_auc, const float* d_ndcg, const float* d_rec, int64_t q0, int64_t nq, int nat,
                      float* auc, float* ndcg, float* recall) {
    if (auc) ORX_HIP(hipMemcpyAsync(auc + q0, d_auc, sizeof(float) * nq, hipMemcpyDeviceToHost, c->stream));
    if (ndcg) ORX_HIP(hipMemcpyAsync(ndcg + (size_t)q0 * nat, d_ndcg, sizeof(float) * nq * nat, hipMemcpyDeviceToHost, c->stream));
    if (recall) ORX_HIP(hipMemcpyAsync(recall + (size_t)q0 * nat, d_rec, sizeof(float) * nq * nat, hipMemcpyDeviceToHost, c->stream));
    return ORX_OK;
}

// ---- the one CSR metrics batch ----------------------------------------------------------------------------------------------
int orx_rank_csr_run(orx_ctx* c, const RankCsrCall& k, int64_t q0, int64_t nq) {
    const int64_t items = k.items, W = (items + 31) / 32;
    const int nat = k.nat;
    const bool scorer = k.pred == nullptr, dev_pred = k.pred && k.pred_on_device;
    const int64_t rows = scorer ? orx_dense_rows(k.n, nq) : nq;
    const size_t cells = (size_t)nq * items;
    const int S = orx_rank_csr_segments(nq, items);
    const int64_t npos = k.pos_ptr[q0 + nq] - k.pos_ptr[q0], nexcl = k.excl_ptr[q0 + nq] - k.excl_ptr[q0];
    // one upload: pos_ptr [nq+1] | excl_ptr [nq+1] (int64, from 0) | pos_items | excl_items (int32) | at [16] (float)
    const size_t up_bytes = 2 * (size_t)(nq + 1) * 8 + ((size_t)npos + nexcl + ORX_EVAL_NAT) * 4;
    // one download: auc [nq] | ndcg [nq nat] | recall [nq nat] | error flag
    const size_t nout = (size_t)nq * (1 + 2 * nat) + 1;
    static thread_local std::vector<char> pack;
    pack.resize(std::max(up_bytes, nout * 4));
    {
        int64_t* hp = (int64_t*)pack.data(); int64_t* he = hp + (nq + 1);
        char* h = (char*)(he + (nq + 1));
        orx_pack_csr(k.pos_ptr, k.pos_items, q0, nq, hp, h);
        h += 4 * (size_t)npos;
        orx_pack_csr(k.excl_ptr, k.excl_items, q0, nq, he, h);
        h += 4 * (size_t)nexcl;
        memset(h, 0, 4 * ORX_EVAL_NAT); memcpy(h, k.at, sizeof(float) * nat);
    }
    // d_dflag: the upload | partials [nq S 136] | n_eval [nq] | results [nout];  d_evalbits: the two bitmaps [2 nq W], all zero between calls
    ENSURE(c->d_dflag, c->d_dflag_cap, up_bytes + ((size_t)nq * S * 136 + nq + nout) * 4);
    const size_t bit_bytes = 2 * (size_t)nq * W * 4;
    CHECK(orx_evalbits_reserve(c, bit_bytes));
    if (!dev_pred) ENSURE(c->d_tmp, c->d_tmp_cap, (size_t)rows * items * sizeof(float));
    float* d_pred = dev_pred ? const_cast<float*>(k.pred) + (size_t)q0 * items : c->d_tmp;
    int64_t* d_pp = (int64_t*)c->d_dflag; int64_t* d_ep = d_pp + (nq + 1);
    int32_t* d_pi = (int32_t*)(d_ep + (nq + 1)); int32_t* d_ei = d_pi + npos;
    float* d_at = (float*)(d_ei + nexcl);
    unsigned* d_part = (unsigned*)(d_at + ORX_EVAL_NAT); int* d_neval = (int*)(d_part + (size_t)nq * S * 136);
    float* d_auc = (float*)(d_neval + nq); float* d_ndcg = d_auc + nq; float* d_rec = d_ndcg + (size_t)nq * nat;
    int* d_flag = (int*)(d_rec + (size_t)nq * nat);
    ORX_HIP(hipMemcpyAsync(c->d_dflag, pack.data(), up_bytes, hipMemcpyHostToDevice, c->stream));
    EvalCsrArgs a;
    a.pred = d_pred; a.pbits = c->d_evalbits; a.ebits = c->d_evalbits + (size_t)nq * W; a.pos_ptr = d_pp; a.pos_items = d_pi;
    a.excl_ptr = d_ep; a.excl_items = d_ei; a.NI = items; a.W = W; a.at = d_at; a.nat = nat;
    a.auc = d_auc; a.ndcg = d_ndcg; a.recall = d_rec; a.err = c->d_err; a.part = d_part; a.neval = d_neval; a.S = S;
    a.flag_out = d_flag; a.q0 = 0;
    // Everything that can fail without touching the bitmaps comes FIRST: the bitmaps are all zero between calls, the first
    // orx_launch_mask_bits sets bits and only the last one clears them again -- an early return in between would leave every later
    // evaluation on this context with stale masks.
    if (scorer) CHECK(orx_stage_uid_rows(c, k.uid + q0, nq, rows));
    CHECK(orx_launch_mask_bits(c, a, nq, 0));
    // ... and whatever fails from here on clears them before it leaves
    auto body = [&]() -> int {
        // (scoring and sweeping slices of the batch on two streams -- a write stream beside a read stream -- was measured and is
        // slower at every slice count: profiles/r3_eval_notes.txt)
        if (scorer)
            CHECK(orx_launch_score_all(c, k.U->w, k.V->w, k.b ? k.b->w : nullptr, k.w ? k.w->w : nullptr, c->d_ids, rows, k.U->rows, items,
                                       k.U->dim, k.kind, d_pred));
        else if (!dev_pred)
            ORX_HIP(hipMemcpyAsync(d_pred, k.pred + (size_t)q0 * items, cells * sizeof(float), hipMemcpyHostToDevice, c->stream));
        return orx_launch_rank_sweeps(c, a, 0, nq, k.max_pos);
    };
    const int body_rc = body();
    if (body_rc != ORX_OK) {
        hipMemsetAsync(c->d_evalbits, 0, bit_bytes, c->stream);
        return body_rc;
    }
    CHECK(orx_launch_mask_bits(c, a, nq, 1));
    ORX_HIP(hipMemcpyAsync(pack.data(), d_auc, nout * 4, hipMemcpyDeviceToHost, c->stream));
    ORX_HIP(hipStreamSynchronize(c->stream));
    const float* r = (const float*)pack.data();
    if (k.auc) memcpy(k.auc + q0, r, sizeof(float) * nq);
    if (k.ndcg) memcpy(k.ndcg + (size_t)q0 * nat, r + nq, sizeof(float) * nq * nat);
    if (k.recall) memcpy(k.recall + (size_t)q0 * nat, r + nq + (size_t)nq * nat, sizeof(float) * nq * nat);
    int flag; memcpy(&flag, r + nout - 1, sizeof(int));
    // (3 is out of reach of orx_rank_metrics_matrixfree: its lists have been checked strictly ascending on the host)
    ORX_ARG(flag != 3, "%s: a user's positive list repeats an item (the lists are sets)", k.fn);
    if (flag) {
        orx_set_error("id out of range: an index in the batch is < 0 or >= the table's row count");
        return ORX_ERR_INDEX;
    }
    return ORX_OK;
}

// ---- entry points ---------------------------------------------------------------------------------------------------------
// scores of the given users against all items: to the host through d_tmp, or left in device memory (out [n, item_rows] fp32: what
// the metrics of the evaluation step read)
static int score_all_items(const char* fn, orx_ctx* c, int kind, orx_table* U, orx_table* V, orx_table* b, orx_table* w,
                           const int32_t* uid, int64_t n, float* out, bool out_on_device) {
    CHECK(orx_sync_tables({U, V, b, w}));
    ORX_ARG(c && U && V && (n == 0 || (uid && out)), "%s: NULL argument", fn);
    CHECK(orx_check_scorer(fn, c, kind, U, V, b, w, uid, n, false));
    if (n == 0) return ORX_OK;
    ORX_HIP(hipSetDevice(c->device));
    const size_t bytes = (size_t)n * V->rows * sizeof(float);
    if (!out_on_device) ENSURE(c->d_tmp, c->d_tmp_cap, bytes);
    float* d_out = out_on_device ? out : c->d_tmp;
    CHECK(orx_stage_uid_rows(c, uid, n, n));
    CHECK(orx_launch_score_all(c, U->w, V->w, b ? b->w : nullptr, w ? w->w : nullptr, c->d_ids, n, U->rows, V->rows, U->dim, kind, d_out));
    if (!out_on_device) ORX_HIP(hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, c->stream));
    return orx_check_index_error(c);
}

extern "C" int orx_score_all_items(orx_ctx* c, int kind, orx_table* U, orx_table* V, orx_table* b, orx_table* w,
                                   const int32_t* uid, int64_t n, float* out) {
    return score_all_items("orx_score_all_items", c, kind, U, V, b, w, uid, n, out, false);
}

extern "C" int orx_score_all_items_device(orx_ctx* c, int kind, orx_table* U, orx_table* V, orx_table* b, orx_table* w,
                                          const int32_t* uid, int64_t n, float* out_dev) {
    return score_all_items("orx_score_all_items_device", c, kind, U, V, b, w, uid, n, out_dev, true);
}

extern "C" int orx_rank_metrics(orx_ctx* c, int kind, orx_table* U, orx_table* V, orx_table* b, orx_table* w,
                                const int32_t* uid, const float* pred, const uint8_t* pos_mask, const uint8_t* excl_mask,
                                int64_t n, int64_t items, const float* at, int32_t nat,
                                float* auc, float* ndcg, float* recall) {
    static const char* fn = "orx_rank_metrics";
    CHECK(orx_sync_tables({U, V, b, w}));
    ORX_ARG(c && pos_mask && excl_mask && at, "%s: NULL argument", fn);
    ORX_ARG(nat >= 1 && nat <= ORX_EVAL_NAT, "%s: nat must be in [1, 16]", fn);
    ORX_ARG(pred || (U && V && uid), "%s: need either pred or tables + user ids", fn);
    ORX_ARG(pred || V->rows == items, "%s: items must equal the item table's rows", fn);
    if (n == 0) return ORX_OK;
    if (!pred) CHECK(orx_check_scorer(fn, c, kind, U, V, b, w, uid, n, false));
    ORX_HIP(hipSetDevice(c->device));
    const size_t cells = (size_t)n * items;
    // layout of d_tmp: pred [cells] | auc [n] | ndcg [n*nat] | recall [n*nat] | at [nat]
    const size_t nf = cells + (size_t)n * (1 + 2 * nat) + nat;
    ENSURE(c->d_tmp, c->d_tmp_cap, nf * sizeof(float));
    ENSURE(c->d_dflag, c->d_dflag_cap, 2 * cells);
    float* d_pred = c->d_tmp; float* d_auc = d_pred + cells; float* d_ndcg = d_auc + n; float* d_rec = d_ndcg + (size_t)n * nat;
    float* d_at = d_rec + (size_t)n * nat;
    unsigned char* d_pos = c->d_dflag; unsigned char* d_excl = d_pos + cells;
    ORX_HIP(hipMemcpyAsync(d_pos, pos_mask, cells, hipMemcpyHostToDevice, c->stream));
    ORX_HIP(hipMemcpyAsync(d_excl, excl_mask, cells, hipMemcpyHostToDevice, c->stream));
    ORX_HIP(hipMemcpyAsync(d_at, at, sizeof(float) * nat, hipMemcpyHostToDevice, c->stream));
    if (pred) {
        ORX_HIP(hipMemcpyAsync(d_pred, pred, cells * sizeof(float), hipMemcpyHostToDevice, c->stream));
    } else {
        CHECK(orx_stage_uid_rows(c, uid, n, n));
        CHECK(orx_launch_score_all(c, U->w, V->w, b ? b->w : nullptr, w ? w->w : nullptr, c->d_ids, n, U->rows, V->rows, U->dim, kind, d_pred));
    }
    EvalArgs a;
    a.pred = d_pred; a.pos = d_pos; a.excl = d_excl; a.NI = items; a.at = d_at; a.nat = nat;
    a.auc = d_auc; a.ndcg = d_ndcg; a.recall = d_rec; a.err = c->d_err;
    CHECK(orx_launch_rank_metrics(c, a, n));
    CHECK(orx_fetch_metrics(c, d_auc, d_ndcg, d_rec, 0, n, nat, auc, ndcg, recall));
    ORX_HIP(hipStreamSynchronize(c->stream));
    int flag = 0;
    ORX_HIP(hipMemcpy(&flag, c->d_err, sizeof(int), hipMemcpyDeviceToHost));
    if (flag == 2) {
        ORX_HIP(hipMemset(c->d_err, 0, sizeof(int)));
        orx_set_error("%s: a user has more than 8192 positive items", fn);
        return ORX_ERR_ARG;
    }
    return orx_check_index_error(c);
}

// The same metrics with the masks as CSR lists over the call's users (pos_ptr / excl_ptr: host int64[n + 1] starting at 0).
extern "C" int orx_rank_metrics_csr(orx_ctx* c, int kind, orx_table* U, orx_table* V, orx_table* b, orx_table* w,
                                    const int32_t* uid, const float* pred, int32_t pred_on_device, int64_t n, int64_t items,
                                    const int64_t* pos_ptr, const int32_t* pos_items, const int64_t* excl_ptr, const int32_t* excl_items,
                                    const float* at, int32_t nat, float* auc, float* ndcg, float* recall) {
    static const char* fn = "orx_rank_metrics_csr";
    CHECK(orx_sync_tables({U, V, b, w}));
    ORX_ARG(c && pos_ptr && excl_ptr && at && n >= 0 && items > 0, "%s: NULL argument", fn);
    ORX_ARG(nat >= 1 && nat <= ORX_EVAL_NAT, "%s: nat must be in [1, 16]", fn);
    ORX_ARG(pred || (U && V && uid), "%s: need either pred or tables + user ids", fn);
    ORX_ARG(pred || V->rows == items, "%s: items must equal the item table's rows", fn);
    if (n == 0) return ORX_OK;
    // (the ids of these lists are checked on the device, by the kernel that sets their bits)
    ORX_ARG(pos_ptr[0] == 0 && excl_ptr[0] == 0, "%s: the lists start at offset 0", fn);
    int64_t max_pos = 0;
    for (int64_t q = 0; q < n; ++q) {
        const int64_t lp = pos_ptr[q + 1] - pos_ptr[q], le = excl_ptr[q + 1] - excl_ptr[q];
        ORX_ARG(lp >= 0 && le >= 0, "%s: offsets must not decrease", fn);
        if (lp > max_pos) max_pos = lp;
    }
    ORX_ARG((pos_ptr[n] == 0 || pos_items) && (excl_ptr[n] == 0 || excl_items), "%s: NULL item list", fn);
    if (!pred) CHECK(orx_check_scorer(fn, c, kind, U, V, b, w, uid, n, false));
    ORX_HIP(hipSetDevice(c->device));
    const RankCsrCall k = {fn, kind, U, V, b, w, uid, pred, pred_on_device != 0, n, items, pos_ptr, pos_items, excl_ptr, excl_items,
                           at, nat, max_pos, auc, ndcg, recall};
    return orx_rank_csr_run(c, k, 0, n);
}
