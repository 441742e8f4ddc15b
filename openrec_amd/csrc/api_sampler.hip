// C-ABI entry points of the device sampler: every orx_sampler_* call and the host-only alias-table builder orx_alias_build
// (include/openrec_hip.h has the contract; kernels_sampler.hip, kernels_hardneg.hip and kernels_warp.hip the kernels, DESIGN.md
// 4.5s what is shared).  A producer checks its window and its own ranges, fills a SamplerArgs through sampler_args -- the one place
// that does -- and launches; the producers that score (pairwise_hard, pairwise_warp) share check_sampler_scorer and sync_scorer.
// What an entry point accepts at n == 0 and where it returns before hipSetDevice is its own and stays as it was.
#include <climits>
#include <cmath>
#include <cstring>

#include "orx_internal.h"

namespace {

// Every field, from the sampler and the call.  The pointwise producers pass their item buffer as pid and no nid.
SamplerArgs sampler_args(orx_sampler* s, uint64_t seed, int64_t first, int64_t n, int32_t* uid, int32_t* pid, int32_t* nid) {
    SamplerArgs a;
    a.rec_user = s->rec_user; a.rec_item = s->rec_item; a.R = s->R; a.ptr = s->ptr; a.items = s->items;
    a.total_items = s->total_items; a.total_users = s->total_users; a.seed = seed; a.first = first; a.n = n; a.h = s->h;
    a.uid = uid; a.pid = pid; a.nid = nid;
    a.prop = s->prop_on ? s->d_prop : nullptr;
    return a;
}

// the sampler, the window and the output buffers a producer cannot do without; `even_empty`: it wants them at n == 0 too
int check_window(const char* fn, orx_sampler* s, int64_t first, int64_t n, bool even_empty, std::initializer_list<const void*> outs) {
    bool have = true;
    for (const void* p : outs) have = have && p;
    ORX_ARG(s && first >= 0 && n >= 0 && (have || (n == 0 && !even_empty)), "%s: bad argument", fn);
    return ORX_OK;
}

int check_no_proposal(const char* fn, orx_sampler* s) {
    ORX_ARG(!s->prop_on, "%s: a proposal is set (orx_sampler_set_proposal) and the pointwise producers draw "
            "uniform negatives only; set it to NULL first", fn);
    return ORX_OK;
}

// the model a producer scores its candidates with: kind, context, row counts, dims, the bias shape
int check_sampler_scorer(const char* fn, orx_sampler* s, int model, orx_table* user, orx_table* item, orx_table* bias) {
    ORX_ARG(model == ORX_BPR || model == ORX_UCML, "%s: the model must be ORX_BPR or ORX_UCML, got %d", fn, model);
    ORX_ARG(user->ctx == s->ctx && item->ctx == s->ctx && (!bias || bias->ctx == s->ctx),
            "%s: the tables live on another context than the sampler", fn);
    ORX_ARG(user->rows == s->total_users, "%s: the user table has %lld rows, the sampler %lld users", fn, (long long)user->rows,
            (long long)s->total_users);
    ORX_ARG(item->rows == s->total_items, "%s: the item table has %lld rows, the sampler %lld items", fn, (long long)item->rows,
            (long long)s->total_items);
    ORX_ARG(user->dim == item->dim, "%s: user dim %d, item dim %d", fn, user->dim, item->dim);
    ORX_ARG(!bias || (bias->rows == s->total_items && bias->dim == 1), "%s: the bias must be [items, 1]", fn);
    return ORX_OK;
}

// the kernel gathers rows the host does not know (they are drawn on the device): the WHOLE of a lazily-applied table is finished
int sync_scorer(orx_table* user, orx_table* item, orx_table* bias) {
    CHECK(orx_table_sync(user));
    CHECK(orx_table_sync(item));
    return orx_table_sync(bias);
}

// One of the device copies a sampler keeps (d_prop, d_recw, d_warpw): allocated on first use at `cap` bytes, the size the sampler
// fixes, then `bytes` of it overwritten.  Launches enqueued before the call read the old copy, so the stream is waited for first.
template <class T>
int sampler_upload(orx_sampler* s, T** dev, size_t cap, const void* host, size_t bytes) {
    if (!*dev) ORX_HIP(hipMalloc((void**)dev, cap));
    ORX_HIP(hipStreamSynchronize(s->ctx->stream));
    ORX_HIP(hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice));
    return ORX_OK;
}

int sampler_fill(orx_sampler* s, const int32_t* rec_user, const int32_t* rec_item, const int64_t* csr_ptr, const int32_t* csr_items) {
    const int64_t nnz = csr_ptr[s->total_users];
    ORX_HIP(hipMalloc((void**)&s->rec_user, sizeof(int32_t) * s->R));
    ORX_HIP(hipMalloc((void**)&s->rec_item, sizeof(int32_t) * s->R));
    ORX_HIP(hipMalloc((void**)&s->ptr, sizeof(int64_t) * (s->total_users + 1)));
    ORX_HIP(hipMalloc((void**)&s->items, sizeof(int32_t) * (nnz > 0 ? nnz : 1)));
    ORX_HIP(hipMemcpy(s->rec_user, rec_user, sizeof(int32_t) * s->R, hipMemcpyHostToDevice));
    ORX_HIP(hipMemcpy(s->rec_item, rec_item, sizeof(int32_t) * s->R, hipMemcpyHostToDevice));
    ORX_HIP(hipMemcpy(s->ptr, csr_ptr, sizeof(int64_t) * (s->total_users + 1), hipMemcpyHostToDevice));
    if (nnz > 0) ORX_HIP(hipMemcpy(s->items, csr_items, sizeof(int32_t) * nnz, hipMemcpyHostToDevice));
    return ORX_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------- the object ---
extern "C" int orx_sampler_create(orx_ctx* ctx, const int32_t* rec_user, const int32_t* rec_item, int64_t n_records,
                                  const int64_t* csr_ptr, const int32_t* csr_items, int64_t total_users, int64_t total_items,
                                  orx_sampler** out) {
    ORX_ARG(ctx && rec_user && rec_item && csr_ptr && csr_items && out, "orx_sampler_create: NULL argument");
    ORX_ARG(n_records > 0 && total_users > 0 && total_items > 0, "orx_sampler_create: sizes must be positive");
    ORX_HIP(hipSetDevice(ctx->device));
    orx_sampler* s = new orx_sampler();
    s->ctx = ctx; s->R = n_records; s->total_users = total_users; s->total_items = total_items;
    while ((1ll << (2 * s->h)) < n_records) s->h++;
    const int rc = sampler_fill(s, rec_user, rec_item, csr_ptr, csr_items);
    if (rc != ORX_OK) { orx_sampler_destroy(s); return rc; }      // (nothing of a half-built sampler is left behind)
    *out = s;
    return ORX_OK;
}

extern "C" int orx_sampler_destroy(orx_sampler* s) {
    if (!s) return ORX_OK;
    hipSetDevice(s->ctx->device);
    hipStreamSynchronize(s->ctx->stream);
    hipFree(s->rec_user); hipFree(s->rec_item); hipFree(s->ptr); hipFree(s->items);
    hipFree(s->d_counter); hipFree(s->d_blockcnt); hipFree(s->d_blockbase); hipFree(s->d_prop); hipFree(s->d_recw);
    hipFree(s->d_warpw);
    delete s;
    return ORX_OK;
}

// ------------------------------------------------------------------------------ the proposal and the record weights ---
// Vose's construction in double.  p[i] = n w[i] / sum(w) is the mass of item i in units of a column.  A column of p < 1 is
// closed by the overflow of a column of p >= 1, which loses that much.  Items of weight 0 are closed FIRST, while a column with
// overflow is certain to exist (the others sum to n over fewer than n columns), so no rounding can leave one of them over: a
// column that is left over keeps all its mass, which would hand such an item 1 / n.  Should it happen all the same, the column
// goes to the heaviest item as a whole.  Only columns of p >= 1 at the time are ever aliased to, so never an item of weight 0.
extern "C" int orx_alias_build(const double* weights, int64_t n, uint32_t* thr_out, int32_t* alias_out) {
    ORX_ARG(weights && thr_out && alias_out, "orx_alias_build: NULL argument");
    ORX_ARG(n >= 1 && n <= (int64_t)INT32_MAX, "orx_alias_build: n must be in [1, 2^31 - 1], got %lld", (long long)n);
    double sum = 0.0; int64_t heaviest = 0;
    for (int64_t i = 0; i < n; ++i) {
        const double w = weights[i];
        ORX_ARG(std::isfinite(w) && w >= 0.0, "orx_alias_build: weight %lld is %g (weights are finite and >= 0)", (long long)i, w);
        sum += w;
        if (w > weights[heaviest]) heaviest = i;
    }
    ORX_ARG(sum > 0.0 && std::isfinite(sum), "orx_alias_build: the weights sum to %g (some weight must be positive, the sum finite)", sum);
    std::vector<double> p((size_t)n);
    std::vector<int32_t> small, large;      // stacks
    small.reserve((size_t)n); large.reserve((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        p[i] = weights[i] / sum * (double)n;
        if (p[i] >= 1.0) large.push_back((int32_t)i);
        else if (weights[i] > 0.0) small.push_back((int32_t)i);
    }
    for (int64_t i = 0; i < n; ++i)        // on top of the stack: closed first
        if (weights[i] == 0.0) small.push_back((int32_t)i);
    auto close = [&](int32_t s, int32_t l) {
        // threshold = p[s] in units of 2^-32, rounded to nearest; a column that rounds to the whole keeps all its mass
        const double q = std::floor(p[s] * 4294967296.0 + 0.5);
        if (q >= 4294967296.0) { thr_out[s] = 0xffffffffu; alias_out[s] = s; }
        else { thr_out[s] = q > 0.0 ? (uint32_t)q : 0u; alias_out[s] = l; }
    };
    while (!small.empty() && !large.empty()) {
        const int32_t s = small.back(), l = large.back();
        small.pop_back();
        close(s, l);
        p[l] = (p[l] + p[s]) - 1.0;
        if (p[l] < 1.0) { large.pop_back(); small.push_back(l); }
    }
    for (int32_t l : large) { thr_out[l] = 0xffffffffu; alias_out[l] = l; }
    for (int32_t s : small) {               // left over through rounding: p[s] is 1 up to that rounding
        if (weights[s] > 0.0) { thr_out[s] = 0xffffffffu; alias_out[s] = s; }
        else { thr_out[s] = 0u; alias_out[s] = (int32_t)heaviest; }
    }
    return ORX_OK;
}

extern "C" int orx_sampler_set_proposal(orx_sampler* s, const double* weights) {
    ORX_ARG(s, "orx_sampler_set_proposal: NULL sampler");
    if (!weights) { s->prop_on = false; return ORX_OK; }      // launches already enqueued carry the table's pointer themselves
    const size_t n = (size_t)s->total_items;
    std::vector<uint32_t> thr(n); std::vector<int32_t> alias(n);
    const int rc = orx_alias_build(weights, s->total_items, thr.data(), alias.data());
    if (rc != ORX_OK) return rc;
    std::vector<uint2> rec(n);
    for (size_t i = 0; i < n; ++i) rec[i] = make_uint2(thr[i], (uint32_t)alias[i]);
    ORX_HIP(hipSetDevice(s->ctx->device));
    CHECK(sampler_upload(s, &s->d_prop, sizeof(uint2) * n, rec.data(), sizeof(uint2) * n));
    s->prop_on = true;
    return ORX_OK;
}

extern "C" int orx_sampler_proposal_read(orx_sampler* s, uint32_t* thr_out, int32_t* alias_out) {
    ORX_ARG(s && thr_out && alias_out, "orx_sampler_proposal_read: NULL argument");
    ORX_ARG(s->prop_on, "orx_sampler_proposal_read: no proposal is set");
    const size_t n = (size_t)s->total_items;
    std::vector<uint2> rec(n);
    ORX_HIP(hipSetDevice(s->ctx->device));
    ORX_HIP(hipStreamSynchronize(s->ctx->stream));
    ORX_HIP(hipMemcpy(rec.data(), s->d_prop, sizeof(uint2) * n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) { thr_out[i] = rec[i].x; alias_out[i] = (int32_t)rec[i].y; }
    return ORX_OK;
}

extern "C" int orx_sampler_set_record_weights(orx_sampler* s, const float* host_w) {
    ORX_ARG(s, "orx_sampler_set_record_weights: NULL sampler");
    if (!host_w) { s->recw_on = false; return ORX_OK; }       // launches already enqueued carry the array's pointer themselves
    ORX_HIP(hipSetDevice(s->ctx->device));
    CHECK(sampler_upload(s, &s->d_recw, sizeof(float) * (size_t)s->R, host_w, sizeof(float) * (size_t)s->R));
    s->recw_on = true;
    return ORX_OK;
}

// ---------------------------------------------------------------------------------------------- the pairwise producers ---
extern "C" int orx_sampler_pairwise(orx_sampler* s, uint64_t seed, int64_t first, int64_t n,
                                    int32_t* uid_dev, int32_t* pid_dev, int32_t* nid_dev) {
    CHECK(check_window("orx_sampler_pairwise", s, first, n, true, {uid_dev, pid_dev, nid_dev}));
    ORX_HIP(hipSetDevice(s->ctx->device));
    return orx_launch_sample_pairwise(s->ctx, sampler_args(s, seed, first, n, uid_dev, pid_dev, nid_dev));
}

extern "C" int orx_sampler_pairwise_weights(orx_sampler* s, uint64_t seed, int64_t first, int64_t n, float* w_dev) {
    CHECK(check_window("orx_sampler_pairwise_weights", s, first, n, false, {w_dev}));
    if (!s->recw_on) {
        orx_set_error("orx_sampler_pairwise_weights: no record weights are set (orx_sampler_set_record_weights)");
        return ORX_ERR_STATE;
    }
    if (n == 0) return ORX_OK;
    ORX_HIP(hipSetDevice(s->ctx->device));
    return orx_launch_sample_weights(s->ctx, sampler_args(s, seed, first, n, nullptr, nullptr, nullptr), s->d_recw, w_dev);
}

extern "C" int orx_sampler_pairwise_multi(orx_sampler* s, uint64_t seed, int64_t first, int64_t n, int32_t n_neg,
                                          int32_t* uid_dev, int32_t* pid_dev, int32_t* nid_dev) {
    static const char* fn = "orx_sampler_pairwise_multi";
    CHECK(check_window(fn, s, first, n, false, {uid_dev, pid_dev, nid_dev}));
    ORX_ARG(n_neg >= 1 && n_neg <= 64, "%s: n_neg must be in [1, 64], got %d", fn, n_neg);
    if (n == 0) return ORX_OK;
    ORX_HIP(hipSetDevice(s->ctx->device));
    return orx_launch_sample_multi(s->ctx, sampler_args(s, seed, first, n, uid_dev, pid_dev, nid_dev), n_neg);
}

extern "C" int orx_sampler_pairwise_hard(orx_sampler* s, int model, orx_table* user, orx_table* item, orx_table* bias,
                                         uint64_t seed, int64_t first, int64_t n, int32_t n_cand,
                                         int32_t* uid_dev, int32_t* pid_dev, int32_t* nid_dev,
                                         int32_t* cand_dev, float* cand_score_dev) {
    static const char* fn = "orx_sampler_pairwise_hard";
    CHECK(check_window(fn, s, first, n, false, {uid_dev, pid_dev, nid_dev}));
    ORX_ARG(user && item, "%s: bad argument", fn);
    ORX_ARG(n_cand >= 1 && n_cand <= 64, "%s: n_cand must be in [1, 64], got %d", fn, n_cand);
    CHECK(check_sampler_scorer(fn, s, model, user, item, bias));
    if (n == 0) return ORX_OK;
    CHECK(sync_scorer(user, item, bias));
    ORX_HIP(hipSetDevice(s->ctx->device));
    HardNegArgs a;
    a.s = sampler_args(s, seed, first, n, uid_dev, pid_dev, nid_dev);
    a.U = user->w; a.V = item->w; a.b = bias ? bias->w : nullptr;
    a.model = model; a.D = user->dim; a.M = n_cand; a.cand = cand_dev; a.cand_score = cand_score_dev;
    return orx_launch_hardneg(s->ctx, a);
}

extern "C" int orx_sampler_pairwise_warp(orx_sampler* s, int model, orx_table* user, orx_table* item, orx_table* bias,
                                         uint64_t seed, int64_t first, int64_t n, int32_t max_trials, float margin,
                                         const float* trial_weight,
                                         int32_t* uid_dev, int32_t* pid_dev, int32_t* nid_dev, float* weight_dev,
                                         int32_t* trials_dev, float* pos_score_dev, float* cand_score_dev) {
    static const char* fn = "orx_sampler_pairwise_warp";
    CHECK(check_window(fn, s, first, n, false, {uid_dev, pid_dev, nid_dev}));
    ORX_ARG(user && item, "%s: bad argument", fn);
    ORX_ARG(n == 0 || weight_dev, "%s: weight_dev is NULL", fn);
    ORX_ARG(trial_weight, "%s: trial_weight is NULL", fn);
    ORX_ARG(max_trials >= 1 && max_trials <= 256, "%s: max_trials must be in [1, 256], got %d", fn, max_trials);
    ORX_ARG(!std::isnan(margin), "%s: the margin is NaN", fn);
    CHECK(check_sampler_scorer(fn, s, model, user, item, bias));
    if (n == 0) return ORX_OK;
    CHECK(sync_scorer(user, item, bias));
    ORX_HIP(hipSetDevice(s->ctx->device));
    // the weight table: uploaded only when its floats (as bits) differ from the copy on the device -- a loop that passes the same
    // table never waits for the stream.  warpw_n is 0 across the copy: a failed one leaves no table that could be taken for current
    if (s->warpw_n < max_trials || std::memcmp(s->h_warpw, trial_weight, sizeof(float) * max_trials) != 0) {
        s->warpw_n = 0;
        CHECK(sampler_upload(s, &s->d_warpw, sizeof(s->h_warpw), trial_weight, sizeof(float) * max_trials));
        std::memcpy(s->h_warpw, trial_weight, sizeof(float) * max_trials);
        s->warpw_n = max_trials;
    }
    WarpNegArgs a;
    a.s = sampler_args(s, seed, first, n, uid_dev, pid_dev, nid_dev);
    a.U = user->w; a.V = item->w; a.b = bias ? bias->w : nullptr;
    a.model = model; a.D = user->dim; a.T = max_trials; a.margin = margin; a.tw = s->d_warpw;
    a.weight = weight_dev; a.trials = trials_dev; a.pos_score = pos_score_dev; a.cand_score = cand_score_dev;
    return orx_launch_warpneg(s->ctx, a);
}

// --------------------------------------------------------------------------------------------- the pointwise producers ---
extern "C" int orx_sampler_stratified(orx_sampler* s, uint64_t seed, int64_t first, int64_t n, float pos_ratio,
                                      int32_t* uid_dev, int32_t* iid_dev, float* label_dev) {
    static const char* fn = "orx_sampler_stratified";
    CHECK(check_window(fn, s, first, n, true, {uid_dev, iid_dev, label_dev}));
    ORX_ARG(pos_ratio >= 0.f && pos_ratio <= 1.f, "%s: pos_ratio must lie in [0, 1]", fn);
    CHECK(check_no_proposal(fn, s));
    ORX_ARG(first == 0 || (first == s->strat_next && seed == s->strat_seed),
            "%s: the stream is sequential (a positive's place in the epoch counts the positives before it): "
            "continue at sample %lld of the same seed, or restart at 0", fn, (long long)s->strat_next);
    ORX_HIP(hipSetDevice(s->ctx->device));
    if (!s->d_counter) ORX_HIP(hipMalloc((void**)&s->d_counter, sizeof(int64_t)));
    if (first == 0) ORX_HIP(hipMemsetAsync(s->d_counter, 0, sizeof(int64_t), s->ctx->stream));
    const size_t nblocks = (size_t)((n + 255) / 256);
    if (s->block_cap < nblocks) {
        ORX_HIP(hipStreamSynchronize(s->ctx->stream));
        hipFree(s->d_blockcnt); hipFree(s->d_blockbase); s->d_blockcnt = nullptr; s->d_blockbase = nullptr; s->block_cap = 0;
        ORX_HIP(hipMalloc((void**)&s->d_blockcnt, sizeof(int) * nblocks));
        ORX_HIP(hipMalloc((void**)&s->d_blockbase, sizeof(int64_t) * nblocks));
        s->block_cap = nblocks;
    }
    s->strat_next = first + n; s->strat_seed = seed;
    return orx_launch_sample_stratified(s->ctx, sampler_args(s, seed, first, n, uid_dev, iid_dev, nullptr), pos_ratio, label_dev,
                                        s->d_blockcnt, s->d_blockbase, s->d_counter);
}

extern "C" int orx_sampler_per_pos_stratified(orx_sampler* s, uint64_t seed, int64_t first, int64_t n, double pos_ratio,
                                              int32_t* uid_dev, int32_t* iid_dev, float* label_dev) {
    static const char* fn = "orx_sampler_per_pos_stratified";
    CHECK(check_window(fn, s, first, n, true, {uid_dev, iid_dev, label_dev}));
    ORX_ARG(pos_ratio > 0.0 && pos_ratio <= 1.0, "%s: pos_ratio must lie in (0, 1]", fn);
    CHECK(check_no_proposal(fn, s));
    // dataset.py:40 computes int((1 - pos_ratio) / pos_ratio) in Python doubles; in fp32 the quotient lands on the other side of
    // an integer for common ratios (0.05: 19 instead of 18; 1/3: 1 instead of 2), i.e. another group size than the reference's
    const int nneg = (int)((1.0 - pos_ratio) / pos_ratio);
    ORX_ARG(nneg + 1 <= s->total_items, "%s: %d negatives per positive need more than %lld items "
            "(random.sample would raise ValueError)", fn, nneg, (long long)s->total_items);
    ORX_HIP(hipSetDevice(s->ctx->device));
    return orx_launch_sample_perpos(s->ctx, sampler_args(s, seed, first, n, uid_dev, iid_dev, nullptr), nneg, label_dev);
}
