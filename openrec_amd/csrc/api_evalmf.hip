// C-ABI entry points of the evaluation without a score matrix: orx_rank_metrics_matrixfree and its host-only scratch query
// (kernels_evalmf.hip has the semantics and the design; the shared host parts are api_eval.hip's).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orx_internal.h"

static constexpr size_t ORX_EVALMF_SCRATCH = (size_t)512 << 20;     // default budget of one batch of users
static constexpr int64_t ORX_EVALMF_MAX_BATCH = 32768;              // (users are a grid dimension of the sweeps)

// ---- the plan both entry points share ------------------------------------------------------------------------------
// matrix-free route: pieces of d_dflag
enum { MF_AT, MF_UID, MF_PP, MF_EP, MF_PI, MF_EI, MF_PS, MF_ES, MF_TS, MF_TEX, MF_HIST, MF_NZ, MF_NEVAL, MF_OUT, MF_PIECES };

struct EvalMfPlan {
    bool dense;                 // L2, dim > 128, ORX_SCORE_SIMPLE: orx_rank_csr_run per batch
    int NB;                     // orx_rank_buckets of the longest positive list
    int64_t nb;                 // users per batch
    size_t off[MF_PIECES];      // matrix-free: offsets into d_dflag
    size_t dflag_bytes;
    size_t bytes;               // all of it
};

static void evalmf_sizes(EvalMfPlan* p, int64_t nb, int64_t n, int64_t items, int64_t max_pos, int64_t max_excl) {
    p->nb = nb;
    const size_t u = (size_t)nb;
    if (!p->dense) {
        const size_t NB = (size_t)p->NB;
        const size_t sz[MF_PIECES] = {64, u * 4, (u + 1) * 8, (u + 1) * 8, u * max_pos * 4, u * max_excl * 4, u * max_pos * 4,
                                      u * max_excl * 4, u * NB * 4, u * NB * 4, u * NB * 8, u * 4, u * 4,
                                      u * (1 + 2 * ORX_EVAL_NAT) * 4};
        p->bytes = p->dflag_bytes = orx_layout(sz, MF_PIECES, p->off);
    } else {
        const size_t W = (size_t)((items + 31) / 32), rows = (size_t)orx_dense_rows(n, nb);
        // partials of a batch of at most nb users: nq S(nq) <= min(8192 + nq, nq S(1))
        const size_t parts = std::min<size_t>(8192 + u, u * (size_t)orx_rank_csr_segments(1, items));
        // d_dflag as orx_rank_csr_run carves it: the upload | partials [nb S 136] | n_eval | results | flag
        p->dflag_bytes = 2 * (u + 1) * 8 + (u * (max_pos + max_excl) + 16) * 4 + (parts * 136 + u + u * (1 + 2 * ORX_EVAL_NAT) + 1) * 4;
        // ... the score rows (d_tmp), the two bitmaps (d_evalbits), the staged user ids (d_ids)
        p->bytes = p->dflag_bytes + rows * items * 4 + 2 * u * W * 4 + rows * 4;
    }
}

static int evalmf_plan(int64_t n, int64_t items, int dim, int kind, int64_t max_pos, int64_t max_excl, size_t scratch_bytes,
                       EvalMfPlan* p) {
    ORX_ARG(n >= 0 && items > 0 && dim > 0, "orx_rank_metrics_matrixfree: sizes must be positive");
    ORX_ARG(kind >= 0 && kind <= 2, "orx_rank_metrics_matrixfree: unknown kind %d", kind);
    ORX_ARG(max_pos >= 0 && max_excl >= 0 && max_pos <= items && max_excl <= items, "orx_rank_metrics_matrixfree: a list longer than the item table");
    const size_t budget = scratch_bytes ? scratch_bytes : ORX_EVALMF_SCRATCH;
    p->dense = kind == 1 || !orx_evalmf_has_tile(dim) || getenv("ORX_SCORE_SIMPLE") != nullptr;
    p->NB = orx_rank_buckets(max_pos);
    // the largest batch within the budget (the sizes grow with the batch); one user when even that is too much
    const int64_t nb = orx_largest_batch(1, std::max<int64_t>(1, std::min(n, ORX_EVALMF_MAX_BATCH)), [&](int64_t m) {
        evalmf_sizes(p, m, n, items, max_pos, max_excl);
        return p->bytes <= budget;
    });
    evalmf_sizes(p, nb, n, items, max_pos, max_excl);
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

extern "C" int orx_rank_metrics_matrixfree_check(int64_t n, int64_t items, const int64_t* pos_ptr, const int32_t* pos_items,
                                                 const int64_t* excl_ptr, const int32_t* excl_items, int64_t* max_pos, int64_t* max_excl) {
    static const char* fn = "orx_rank_metrics_matrixfree";
    ORX_ARG(pos_ptr && excl_ptr && max_pos && max_excl && n >= 0 && items > 0, "%s: NULL argument", fn);
    *max_pos = 0; *max_excl = 0;
    if (n == 0) return ORX_OK;
    CHECK(orx_check_lists(fn, "positive", pos_ptr, pos_items, n, items, true, max_pos));
    return orx_check_lists(fn, "exclusion", excl_ptr, excl_items, n, items, true, max_excl);
}

extern "C" int orx_rank_metrics_matrixfree(orx_ctx* c, int kind, orx_table* U, orx_table* V, orx_table* b, orx_table* w,
                                           const int32_t* uid, int64_t n, const int64_t* pos_ptr, const int32_t* pos_items,
                                           const int64_t* excl_ptr, const int32_t* excl_items, const float* at, int32_t nat,
                                           size_t scratch_bytes, float* auc, float* ndcg, float* recall) {
    static const char* fn = "orx_rank_metrics_matrixfree";
    CHECK(orx_sync_tables({U, V, b, w}));
    ORX_ARG(c && U && V && pos_ptr && excl_ptr && at && n >= 0 && (n == 0 || uid), "%s: NULL argument", fn);
    ORX_ARG(nat >= 1 && nat <= ORX_EVAL_NAT, "%s: nat must be in [1, 16]", fn);
    CHECK(orx_check_scorer(fn, c, kind, U, V, b, w, uid, n, true));
    if (n == 0) return ORX_OK;
    const int64_t NI = V->rows;
    int64_t max_pos = 0, max_excl = 0;
    CHECK(orx_rank_metrics_matrixfree_check(n, NI, pos_ptr, pos_items, excl_ptr, excl_items, &max_pos, &max_excl));
    EvalMfPlan p;
    CHECK(evalmf_plan(n, NI, U->dim, kind, max_pos, max_excl, scratch_bytes, &p));
    ORX_HIP(hipSetDevice(c->device));
    ENSURE(c->d_dflag, c->d_dflag_cap, p.dflag_bytes);
    if (p.dense) {
        // (the first batch is the largest: it sizes d_tmp, d_evalbits and d_ids for the others)
        const RankCsrCall k = {fn, kind, U, V, b, w, uid, nullptr, false, n, NI, pos_ptr, pos_items, excl_ptr, excl_items,
                               at, nat, max_pos, auc, ndcg, recall};
        for (int64_t q0 = 0; q0 < n; q0 += p.nb) CHECK(orx_rank_csr_run(c, k, q0, std::min(p.nb, n - q0)));
        return ORX_OK;
    }
    static thread_local std::vector<int64_t> hp;
    unsigned char* base = c->d_dflag;
    const int NT = p.NB - 1;
    const int chunks = max_pos <= NT ? 1 : (int)((max_pos + NT - 1) / NT);
    float hat[ORX_EVAL_NAT] = {0};
    memcpy(hat, at, sizeof(float) * nat);
    ORX_HIP(hipMemcpyAsync(base + p.off[MF_AT], hat, 64, hipMemcpyHostToDevice, c->stream));
    for (int64_t q0 = 0; q0 < n; q0 += p.nb) {
        const int64_t nq = std::min(p.nb, n - q0);
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
        hp.resize(2 * (nq + 1));
        CsrSlice sp, se;
        ORX_HIP(hipMemcpyAsync((void*)a.uid, uid + q0, (size_t)nq * 4, hipMemcpyHostToDevice, c->stream));
        CHECK(orx_stage_csr(c, pos_ptr, pos_items, q0, nq, hp.data(), nullptr, (int64_t*)a.pos_ptr, (int32_t*)a.pos_items, &sp));
        CHECK(orx_stage_csr(c, excl_ptr, excl_items, q0, nq, hp.data() + nq + 1, nullptr, (int64_t*)a.excl_ptr, (int32_t*)a.excl_items, &se));
        CHECK(orx_launch_evalmf_gather(c, a, kind, std::max(sp.longest, se.longest)));
        // every user of every batch takes the call's chunking: the float sums are added in the order the one-batch call adds them
        for (int ch = 0; ch < chunks; ++ch) CHECK(orx_launch_evalmf_chunk(c, a, kind, ch * NT, ch == chunks - 1));
        CHECK(orx_fetch_metrics(c, a.auc, a.ndcg, a.recall, q0, nq, nat, auc, ndcg, recall));
        ORX_HIP(hipStreamSynchronize(c->stream));          // (the host staging vector is refilled by the next batch)
    }
    return orx_check_index_error(c);
}
