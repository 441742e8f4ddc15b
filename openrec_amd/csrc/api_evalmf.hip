// C-ABI entry points of the evaluation without a score matrix: orx_rank_metrics_matrixfree and its host-only scratch query
// (kernels_evalmf.hip has the semantics and the design).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orx_internal.h"

static constexpr size_t ORX_EVALMF_SCRATCH = (size_t)512 << 20;     // default budget of one batch of users
static constexpr int64_t ORX_EVALMF_MAX_BATCH = 32768;              // (users are a grid dimension of the sweeps)
static constexpr int ORX_EVALMF_NAT = 16;

static size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- the plan both entry points share ------------------------------------------------------------------------------
// matrix-free route: pieces of d_dflag
enum { MF_AT, MF_UID, MF_PP, MF_EP, MF_PI, MF_EI, MF_PS, MF_ES, MF_TS, MF_TEX, MF_HIST, MF_NZ, MF_NEVAL, MF_OUT, MF_PIECES };

struct EvalMfPlan {
    bool dense;                 // L2, dim > 128, ORX_SCORE_SIMPLE: the scorer + the sweeps of orx_rank_metrics_csr per batch
    int NB;                     // buckets: 2^STEPS, STEPS from the longest positive list as rank_sweep_kernel picks it
    int64_t nb;                 // users per batch
    int64_t rows;               // dense: score rows of a batch (at least 65 when n > 64: the scorer's 128-user tile)
    size_t off[MF_PIECES];      // matrix-free: offsets into d_dflag
    size_t dflag_bytes, tmp_bytes, bits_bytes, ids_bytes;
    size_t bytes;               // all of it
};

static void evalmf_sizes(EvalMfPlan* p, int64_t nb, int64_t n, int64_t items, int64_t max_pos, int64_t max_excl) {
    p->nb = nb;
    if (!p->dense) {
        const size_t NB = (size_t)p->NB, u = (size_t)nb;
        const size_t sz[MF_PIECES] = {64, u * 4, (u + 1) * 8, (u + 1) * 8, u * max_pos * 4, u * max_excl * 4, u * max_pos * 4,
                                      u * max_excl * 4, u * NB * 4, u * NB * 4, u * NB * 8, u * 4, u * 4,
                                      u * (1 + 2 * ORX_EVALMF_NAT) * 4};
        size_t total = 0;
        for (int i = 0; i < MF_PIECES; ++i) { p->off[i] = total; total += al256(sz[i]); }
        p->rows = 0; p->dflag_bytes = total; p->tmp_bytes = 0; p->bits_bytes = 0; p->ids_bytes = 0;
    } else {
        const size_t u = (size_t)nb, W = (size_t)((items + 31) / 32);
        // partials of a batch of at most nb users: nq S(nq) <= min(8192 + nq, nq S(1))
        const size_t parts = std::min<size_t>(8192 + u, u * (size_t)orx_rank_csr_segments(1, items));
        p->rows = n > 64 ? std::max<int64_t>(nb, 65) : nb;
        // d_dflag as in orx_rank_metrics_csr: the upload | partials [nb S 136] | n_eval | results | flag
        p->dflag_bytes = 2 * (u + 1) * 8 + (u * (max_pos + max_excl) + 16) * 4 + (parts * 136 + u + u * (1 + 2 * ORX_EVALMF_NAT) + 1) * 4;
        p->tmp_bytes = (size_t)p->rows * items * 4;
        p->bits_bytes = 2 * u * W * 4;
        p->ids_bytes = (size_t)p->rows * 4;
    }
    p->bytes = p->dflag_bytes + p->tmp_bytes + p->bits_bytes + p->ids_bytes;
}

static int evalmf_plan(int64_t n, int64_t items, int dim, int kind, int64_t max_pos, int64_t max_excl, size_t scratch_bytes,
                       EvalMfPlan* p) {
    ORX_ARG(n >= 0 && items > 0 && dim > 0, "orx_rank_metrics_matrixfree: sizes must be positive");
    ORX_ARG(kind >= 0 && kind <= 2, "orx_rank_metrics_matrixfree: unknown kind %d", kind);
    ORX_ARG(max_pos >= 0 && max_excl >= 0 && max_pos <= items && max_excl <= items, "orx_rank_metrics_matrixfree: a list longer than the item table");
    const size_t budget = scratch_bytes ? scratch_bytes : ORX_EVALMF_SCRATCH;
    p->dense = kind == 1 || !orx_evalmf_has_tile(dim) || getenv("ORX_SCORE_SIMPLE") != nullptr;
    p->NB = max_pos <= 7 ? 8 : (max_pos <= 15 ? 16 : 64);
    // the largest batch within the budget (the sizes grow with the batch); one user when even that is too much
    int64_t lo = 1, hi = std::max<int64_t>(1, std::min(n, ORX_EVALMF_MAX_BATCH));
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) / 2;
        evalmf_sizes(p, mid, n, items, max_pos, max_excl);
        if (p->bytes <= budget) lo = mid; else hi = mid - 1;
    }
    evalmf_sizes(p, lo, n, items, max_pos, max_excl);
    for (int guard = 0; p->bytes > budget && p->nb > 1 && guard < 64; ++guard)       // (the dense partials are not quite monotone)
        evalmf_sizes(p, p->nb - 1, n, items, max_pos, max_excl);
    return ORX_OK;
}

extern "C" int orx_rank_metrics_matrixfree_scratch(int64_t n, int64_t items, int32_t dim, int32_t kind, int64_t max_pos,
                                                   int64_t max_excl, size_t scratch_bytes, int64_t* bytes, int64_t* users_per_batch) {
    ORX_ARG(bytes && users_per_batch, "orx_rank_metrics_matrixfree_scratch: NULL argument");
    EvalMfPlan p;
    CHECK(evalmf_plan(n, items, dim, kind, max_pos, max_excl, scratch_bytes, &p));
    *bytes = (int64_t)p.bytes;
    *users_per_batch = p.nb;
    return ORX_OK;
}

// ---- argument checks, all on the host ---------------------------------------------------------------------------------
static int evalmf_check_lists(const char* what, const int64_t* ptr, const int32_t* items, int64_t n, int64_t NI, int64_t* longest) {
    ORX_ARG(ptr[0] == 0, "orx_rank_metrics_matrixfree: the %s lists start at offset 0", what);
    *longest = 0;
    for (int64_t q = 0; q < n; ++q) {
        ORX_ARG(ptr[q + 1] >= ptr[q], "orx_rank_metrics_matrixfree: %s offsets must not decrease", what);
        *longest = std::max(*longest, ptr[q + 1] - ptr[q]);
    }
    ORX_ARG(ptr[n] == 0 || items, "orx_rank_metrics_matrixfree: NULL %s item list", what);
    for (int64_t q = 0; q < n; ++q) {
        for (int64_t i = ptr[q]; i < ptr[q + 1]; ++i) {
            if (items[i] < 0 || items[i] >= NI) {
                orx_set_error("orx_rank_metrics_matrixfree: %s id %d of user %lld outside [0, %lld)", what, items[i], (long long)q, (long long)NI);
                return ORX_ERR_INDEX;
            }
            ORX_ARG(i == ptr[q] || items[i] > items[i - 1],
                    "orx_rank_metrics_matrixfree: the %s list of user %lld is not strictly ascending (item %d after %d)", what,
                    (long long)q, items[i], i == ptr[q] ? 0 : items[i - 1]);
        }
    }
    return ORX_OK;
}

extern "C" int orx_rank_metrics_matrixfree_check(int64_t n, int64_t items, const int64_t* pos_ptr, const int32_t* pos_items,
                                                 const int64_t* excl_ptr, const int32_t* excl_items, int64_t* max_pos, int64_t* max_excl) {
    ORX_ARG(pos_ptr && excl_ptr && max_pos && max_excl && n >= 0 && items > 0, "orx_rank_metrics_matrixfree: NULL argument");
    *max_pos = 0; *max_excl = 0;
    if (n == 0) return ORX_OK;
    CHECK(evalmf_check_lists("positive", pos_ptr, pos_items, n, items, max_pos));
    return evalmf_check_lists("exclusion", excl_ptr, excl_items, n, items, max_excl);
}

// ---- one batch on the dense route: orx_rank_metrics_csr's steps over nq users -----------------------------------------------
static int evalmf_dense_batch(orx_ctx* c, int kind, orx_table* U, orx_table* V, orx_table* b, orx_table* w, const int32_t* uid,
                              int64_t q0, int64_t nq, int64_t rows, const int64_t* pos_ptr, const int32_t* pos_items,
                              const int64_t* excl_ptr, const int32_t* excl_items, const float* at, int nat, int64_t max_pos,
                              float* auc, float* ndcg, float* recall, std::vector<char>& pack, std::vector<int32_t>& huid) {
    const int64_t items = V->rows, W = (items + 31) / 32;
    const int S = orx_rank_csr_segments(nq, items);
    const int64_t pb = pos_ptr[q0], eb = excl_ptr[q0], npos = pos_ptr[q0 + nq] - pb, nexcl = excl_ptr[q0 + nq] - eb;
    const size_t up_bytes = 2 * (size_t)(nq + 1) * 8 + ((size_t)npos + nexcl + 16) * 4;
    const size_t nout = (size_t)nq * (1 + 2 * nat) + 1;
    pack.resize(std::max(up_bytes, nout * 4));
    {
        int64_t* hp = (int64_t*)pack.data(); int64_t* he = hp + (nq + 1);
        for (int64_t q = 0; q <= nq; ++q) { hp[q] = pos_ptr[q0 + q] - pb; he[q] = excl_ptr[q0 + q] - eb; }
        char* h = (char*)(he + (nq + 1));
        if (npos) memcpy(h, pos_items + pb, 4 * (size_t)npos);
        h += 4 * (size_t)npos;
        if (nexcl) memcpy(h, excl_items + eb, 4 * (size_t)nexcl);
        h += 4 * (size_t)nexcl;
        memset(h, 0, 64); memcpy(h, at, sizeof(float) * nat);
    }
    huid.assign(uid + q0, uid + q0 + nq);
    huid.resize(rows, uid[q0]);                       // rows beyond the batch: the scorer's wide tile, their scores are never read
    int64_t* d_pp = (int64_t*)c->d_dflag; int64_t* d_ep = d_pp + (nq + 1);
    int32_t* d_pi = (int32_t*)(d_ep + (nq + 1)); int32_t* d_ei = d_pi + npos;
    float* d_at = (float*)(d_ei + nexcl);
    unsigned* d_part = (unsigned*)(d_at + 16); int* d_neval = (int*)(d_part + (size_t)nq * S * 136);
    float* d_auc = (float*)(d_neval + nq); float* d_ndcg = d_auc + nq; float* d_rec = d_ndcg + (size_t)nq * nat;
    int* d_flag = (int*)(d_rec + (size_t)nq * nat);
    ORX_HIP(hipMemcpyAsync(c->d_dflag, pack.data(), up_bytes, hipMemcpyHostToDevice, c->stream));
    CHECK(stage_ids(c, huid.data(), rows, 0));
    EvalCsrArgs a;
    a.pred = c->d_tmp; a.pbits = c->d_evalbits; a.ebits = c->d_evalbits + (size_t)nq * W; a.pos_ptr = d_pp; a.pos_items = d_pi;
    a.excl_ptr = d_ep; a.excl_items = d_ei; a.NI = items; a.W = W; a.at = d_at; a.nat = nat;
    a.auc = d_auc; a.ndcg = d_ndcg; a.recall = d_rec; a.err = c->d_err; a.part = d_part; a.neval = d_neval; a.S = S;
    a.flag_out = d_flag; a.q0 = 0;
    // the bitmaps are all zero between calls: whatever fails between setting and clearing them wipes them before it leaves
    CHECK(orx_launch_mask_bits(c, a, nq, 0));
    int rc = orx_launch_score_all(c, U->w, V->w, b ? b->w : nullptr, w ? w->w : nullptr, c->d_ids, rows, U->rows, items, U->dim, kind, c->d_tmp);
    if (rc == ORX_OK) rc = orx_launch_rank_sweeps(c, a, 0, nq, max_pos);
    if (rc != ORX_OK) {
        hipMemsetAsync(c->d_evalbits, 0, 2 * (size_t)nq * W * 4, c->stream);
        return rc;
    }
    CHECK(orx_launch_mask_bits(c, a, nq, 1));
    ORX_HIP(hipMemcpyAsync(pack.data(), d_auc, nout * 4, hipMemcpyDeviceToHost, c->stream));
    ORX_HIP(hipStreamSynchronize(c->stream));
    const float* r = (const float*)pack.data();
    if (auc) memcpy(auc + q0, r, sizeof(float) * nq);
    if (ndcg) memcpy(ndcg + (size_t)q0 * nat, r + nq, sizeof(float) * nq * nat);
    if (recall) memcpy(recall + (size_t)q0 * nat, r + nq + (size_t)nq * nat, sizeof(float) * nq * nat);
    int flag; memcpy(&flag, r + nout - 1, sizeof(int));
    if (flag) {
        orx_set_error("id out of range: an index in the batch is < 0 or >= the table's row count");
        return ORX_ERR_INDEX;
    }
    return ORX_OK;
}

extern "C" int orx_rank_metrics_matrixfree(orx_ctx* c, int kind, orx_table* U, orx_table* V, orx_table* b, orx_table* w,
                                           const int32_t* uid, int64_t n, const int64_t* pos_ptr, const int32_t* pos_items,
                                           const int64_t* excl_ptr, const int32_t* excl_items, const float* at, int32_t nat,
                                           size_t scratch_bytes, float* auc, float* ndcg, float* recall) {
    if (U) CHECK(orx_table_sync(U));
    if (V) CHECK(orx_table_sync(V));
    if (b) CHECK(orx_table_sync(b));
    if (w) CHECK(orx_table_sync(w));
    ORX_ARG(c && U && V && pos_ptr && excl_ptr && at && n >= 0 && (n == 0 || uid), "orx_rank_metrics_matrixfree: NULL argument");
    ORX_ARG(nat >= 1 && nat <= 16, "orx_rank_metrics_matrixfree: nat must be in [1, 16]");
    ORX_ARG(kind >= 0 && kind <= 2 && U->dim == V->dim && U->dim <= 1024, "orx_rank_metrics_matrixfree: bad scorer arguments");
    ORX_ARG(!b || (b->rows == V->rows && b->dim == 1), "orx_rank_metrics_matrixfree: table shapes do not match");
    ORX_ARG(kind != 2 || (w && w->rows == U->dim && w->dim == 1), "orx_rank_metrics_matrixfree: GMF needs w [D, 1]");
    if (n == 0) return ORX_OK;
    const int64_t NI = V->rows;
    int64_t max_pos = 0, max_excl = 0;
    CHECK(orx_rank_metrics_matrixfree_check(n, NI, pos_ptr, pos_items, excl_ptr, excl_items, &max_pos, &max_excl));
    for (int64_t q = 0; q < n; ++q) {
        if (uid[q] < 0 || uid[q] >= U->rows) {
            orx_set_error("orx_rank_metrics_matrixfree: user id %d outside [0, %lld)", uid[q], (long long)U->rows);
            return ORX_ERR_INDEX;
        }
    }
    EvalMfPlan p;
    CHECK(evalmf_plan(n, NI, U->dim, kind, max_pos, max_excl, scratch_bytes, &p));
    ORX_HIP(hipSetDevice(c->device));
    ENSURE(c->d_dflag, c->d_dflag_cap, p.dflag_bytes);
    static thread_local std::vector<char> pack;
    static thread_local std::vector<int32_t> huid;
    static thread_local std::vector<int64_t> hp;
    if (p.dense) {
        ENSURE(c->d_tmp, c->d_tmp_cap, p.tmp_bytes);
        ENSURE(c->d_ids, c->d_ids_cap, p.ids_bytes);
        if (p.bits_bytes > c->d_evalbits_cap) {
            if (c->d_evalbits) ORX_HIP(hipFree(c->d_evalbits));
            c->d_evalbits = nullptr; c->d_evalbits_cap = 0;
            ORX_HIP(hipMalloc((void**)&c->d_evalbits, p.bits_bytes));
            c->d_evalbits_cap = p.bits_bytes;
            ORX_HIP(hipMemsetAsync(c->d_evalbits, 0, p.bits_bytes, c->stream));
        }
        for (int64_t q0 = 0; q0 < n; q0 += p.nb) {
            const int64_t nq = std::min(p.nb, n - q0);
            CHECK(evalmf_dense_batch(c, kind, U, V, b, w, uid, q0, nq, n > 64 ? std::max<int64_t>(nq, 65) : nq, pos_ptr, pos_items,
                                     excl_ptr, excl_items, at, nat, max_pos, auc, ndcg, recall, pack, huid));
        }
        return ORX_OK;
    }
    unsigned char* base = c->d_dflag;
    const int NT = p.NB - 1;
    const int chunks = max_pos <= NT ? 1 : (int)((max_pos + NT - 1) / NT);
    float hat[16] = {0};
    memcpy(hat, at, sizeof(float) * nat);
    ORX_HIP(hipMemcpyAsync(base + p.off[MF_AT], hat, 64, hipMemcpyHostToDevice, c->stream));
    for (int64_t q0 = 0; q0 < n; q0 += p.nb) {
        const int64_t nq = std::min(p.nb, n - q0);
        const int64_t pb = pos_ptr[q0], eb = excl_ptr[q0], npos = pos_ptr[q0 + nq] - pb, nexcl = excl_ptr[q0 + nq] - eb;
        hp.resize(2 * (nq + 1));
        int64_t bmax_pos = 0, bmax_excl = 0;
        for (int64_t q = 0; q <= nq; ++q) { hp[q] = pos_ptr[q0 + q] - pb; hp[nq + 1 + q] = excl_ptr[q0 + q] - eb; }
        for (int64_t q = 0; q < nq; ++q) { bmax_pos = std::max(bmax_pos, hp[q + 1] - hp[q]); bmax_excl = std::max(bmax_excl, hp[nq + 2 + q] - hp[nq + 1 + q]); }
        EvalMfArgs a;
        memset(&a, 0, sizeof(a));
        a.U = U->w; a.V = V->w; a.b = b ? b->w : nullptr; a.w = w ? w->w : nullptr;
        a.uid = (const int32_t*)(base + p.off[MF_UID]); a.nq = nq; a.NU = U->rows; a.NI = NI; a.D = U->dim;
        int KB = 1;
        while (16 * KB < a.D) KB *= 2;
        a.Dp = 16 * KB;
        a.pos_ptr = (const int64_t*)(base + p.off[MF_PP]); a.excl_ptr = (const int64_t*)(base + p.off[MF_EP]);
        a.pos_items = (const int32_t*)(base + p.off[MF_PI]); a.excl_items = (const int32_t*)(base + p.off[MF_EI]);
        a.pos_s = (float*)(base + p.off[MF_PS]); a.excl_s = (float*)(base + p.off[MF_ES]);
        a.ts = (float*)(base + p.off[MF_TS]); a.tex = (int*)(base + p.off[MF_TEX]); a.NB = p.NB;
        a.hist = (unsigned*)(base + p.off[MF_HIST]); a.corr = a.hist + (size_t)nq * p.NB; a.nzdrop = (unsigned*)(base + p.off[MF_NZ]);
        a.at = (const float*)(base + p.off[MF_AT]); a.nat = nat;
        a.neval = (int*)(base + p.off[MF_NEVAL]);
        a.auc = (float*)(base + p.off[MF_OUT]); a.ndcg = a.auc + nq; a.recall = a.ndcg + (size_t)nq * nat;
        a.err = c->d_err;
        ORX_HIP(hipMemcpyAsync((void*)a.uid, uid + q0, (size_t)nq * 4, hipMemcpyHostToDevice, c->stream));
        ORX_HIP(hipMemcpyAsync((void*)a.pos_ptr, hp.data(), (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, c->stream));
        ORX_HIP(hipMemcpyAsync((void*)a.excl_ptr, hp.data() + nq + 1, (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, c->stream));
        if (npos) ORX_HIP(hipMemcpyAsync((void*)a.pos_items, pos_items + pb, (size_t)npos * 4, hipMemcpyHostToDevice, c->stream));
        if (nexcl) ORX_HIP(hipMemcpyAsync((void*)a.excl_items, excl_items + eb, (size_t)nexcl * 4, hipMemcpyHostToDevice, c->stream));
        CHECK(orx_launch_evalmf_gather(c, a, kind, std::max(bmax_pos, bmax_excl)));
        // every user of every batch takes the call's chunking: the float sums are added in the order the one-batch call adds them
        for (int ch = 0; ch < chunks; ++ch) CHECK(orx_launch_evalmf_chunk(c, a, kind, ch * NT, ch == chunks - 1));
        if (auc) ORX_HIP(hipMemcpyAsync(auc + q0, a.auc, sizeof(float) * nq, hipMemcpyDeviceToHost, c->stream));
        if (ndcg) ORX_HIP(hipMemcpyAsync(ndcg + (size_t)q0 * nat, a.ndcg, sizeof(float) * nq * nat, hipMemcpyDeviceToHost, c->stream));
        if (recall) ORX_HIP(hipMemcpyAsync(recall + (size_t)q0 * nat, a.recall, sizeof(float) * nq * nat, hipMemcpyDeviceToHost, c->stream));
        ORX_HIP(hipStreamSynchronize(c->stream));          // (the host staging vector is refilled by the next batch)
    }
    return orx_check_index_error(c);
}
