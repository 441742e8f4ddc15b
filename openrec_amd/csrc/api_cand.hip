// C-ABI entry points of the candidate lists: orx_score_candidates, orx_rank_metrics_candidates and the host-only list check
// (kernels_cand.hip has the semantics and the design; the shared host parts are api_eval.hip's).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orx_internal.h"

static constexpr size_t ORX_CAND_SCRATCH = (size_t)512 << 20;       // default budget of one batch of users
static constexpr int64_t ORX_CAND_MAX_DENSE_BATCH = 32768;          // (users are a grid dimension of the scorer)

extern "C" int orx_rank_metrics_candidates_check(int64_t n, int64_t items, const int64_t* pos_ptr, const int32_t* pos_items,
                                                 const int64_t* cand_ptr, const int32_t* cand_items, int64_t* max_pos,
                                                 int64_t* max_cand) {
    static const char* fn = "orx_rank_metrics_candidates";
    ORX_ARG(pos_ptr && cand_ptr && max_pos && max_cand && n >= 0 && items > 0, "%s: NULL argument", fn);
    *max_pos = 0; *max_cand = 0;
    if (n == 0) return ORX_OK;
    CHECK(orx_check_lists(fn, "positive", pos_ptr, pos_items, n, items, true, max_pos));
    return orx_check_lists(fn, "candidate", cand_ptr, cand_items, n, items, true, max_cand);
}

// ---- the batches both entry points share ----------------------------------------------------------------------------------
// pieces of d_dflag of one batch
enum { CD_AT, CD_UID, CD_PP, CD_CP, CD_PI, CD_CI, CD_PS, CD_CS, CD_OUT, CD_PIECES };

struct CandBatch {
    size_t off[CD_PIECES];
    size_t list_bytes;          // d_dflag
    int64_t rows;               // dense route: score rows (orx_dense_rows)
    size_t bytes;               // all of it
};

static void cand_sizes(CandBatch* p, bool dense, int64_t n, int64_t nq, int64_t npos, int64_t ncand, int64_t items) {
    const size_t u = (size_t)nq;
    const size_t sz[CD_PIECES] = {64, u * 4, (u + 1) * 8, (u + 1) * 8, (size_t)npos * 4, (size_t)ncand * 4, (size_t)npos * 4,
                                  (size_t)ncand * 4, u * (1 + 2 * ORX_EVAL_NAT) * 4};
    p->list_bytes = orx_layout(sz, CD_PIECES, p->off);
    p->rows = dense ? orx_dense_rows(n, nq) : 0;
    p->bytes = p->list_bytes + (size_t)p->rows * items * 4 + (size_t)p->rows * 4;
}

struct CandCall {
    orx_ctx* c; int kind; orx_table* U; orx_table* V; orx_table* b; orx_table* w;
    const int32_t* uid; int64_t n;
    const int64_t* pos_ptr; const int32_t* pos_items;     // NULL: scores only
    const int64_t* cand_ptr; const int32_t* cand_items;
    const float* at; int nat; int NB; size_t budget;
    float* scores; bool scores_on_device;                 // scores only: [cand_ptr[n]]
    float* auc; float* ndcg; float* recall;
};

static int cand_run(const CandCall& k) {
    orx_ctx* c = k.c;
    const int64_t n = k.n, NI = k.V->rows;
    const int D = k.U->dim;
    const bool metrics = k.pos_ptr != nullptr;
    const bool dense = k.kind == 1 || !orx_cand_has_tile(D) || getenv("ORX_SCORE_SIMPLE") != nullptr;
    ORX_HIP(hipSetDevice(c->device));
    static thread_local std::vector<int64_t> hp;
    float hat[ORX_EVAL_NAT] = {0};
    if (metrics) memcpy(hat, k.at, sizeof(float) * k.nat);
    const float* Ub = k.U->w; const float* Vb = k.V->w;
    const float* bb = k.b ? k.b->w : nullptr; const float* wb = k.w ? k.w->w : nullptr;
    for (int64_t q0 = 0; q0 < n;) {
        // the longest run of users whose lists, scores and (dense route) score rows stay within the budget; one user at least
        CandBatch p;
        auto sizes = [&](int64_t m) {
            cand_sizes(&p, dense, n, m, metrics ? k.pos_ptr[q0 + m] - k.pos_ptr[q0] : 0, k.cand_ptr[q0 + m] - k.cand_ptr[q0], NI);
            return p.bytes <= k.budget;
        };
        const int64_t nq = orx_largest_batch(1, dense ? std::min(n - q0, ORX_CAND_MAX_DENSE_BATCH) : n - q0, sizes);   // (the sizes grow with the run)
        sizes(nq);
        const int64_t cb = k.cand_ptr[q0];
        const int64_t npos = metrics ? k.pos_ptr[q0 + nq] - k.pos_ptr[q0] : 0, ncand = k.cand_ptr[q0 + nq] - cb;
        ENSURE(c->d_dflag, c->d_dflag_cap, p.list_bytes);
        unsigned char* base = c->d_dflag;
        int32_t* d_uid = (int32_t*)(base + p.off[CD_UID]);
        int64_t* d_pp = (int64_t*)(base + p.off[CD_PP]); int64_t* d_cp = (int64_t*)(base + p.off[CD_CP]);
        int32_t* d_pi = (int32_t*)(base + p.off[CD_PI]); int32_t* d_ci = (int32_t*)(base + p.off[CD_CI]);
        float* d_ps = (float*)(base + p.off[CD_PS]);
        float* d_cs = (!metrics && k.scores_on_device) ? k.scores + cb : (float*)(base + p.off[CD_CS]);
        hp.resize(2 * (nq + 1));
        ORX_HIP(hipMemcpyAsync(d_uid, k.uid + q0, (size_t)nq * 4, hipMemcpyHostToDevice, c->stream));
        CHECK(orx_stage_csr(c, k.cand_ptr, k.cand_items, q0, nq, hp.data() + nq + 1, nullptr, d_cp, d_ci, nullptr));
        if (metrics) {
            ORX_HIP(hipMemcpyAsync(base + p.off[CD_AT], hat, 64, hipMemcpyHostToDevice, c->stream));
            CHECK(orx_stage_csr(c, k.pos_ptr, k.pos_items, q0, nq, hp.data(), nullptr, d_pp, d_pi, nullptr));
        }
        if (dense) {
            if (npos + ncand > 0) {
                ENSURE(c->d_tmp, c->d_tmp_cap, (size_t)p.rows * NI * 4);
                CHECK(orx_stage_uid_rows(c, k.uid + q0, nq, p.rows));
                CHECK(orx_launch_score_all(c, Ub, Vb, bb, wb, c->d_ids, p.rows, k.U->rows, NI, D, k.kind, c->d_tmp));
                CHECK(orx_launch_cand_pick(c, c->d_tmp, NI, d_cp, d_ci, nq, ncand, d_cs));
                if (metrics) CHECK(orx_launch_cand_pick(c, c->d_tmp, NI, d_pp, d_pi, nq, npos, d_ps));
            }
        } else {
            CandScoreArgs a;
            memset(&a, 0, sizeof(a));
            a.U = Ub; a.V = Vb; a.b = bb; a.w = wb; a.uid = d_uid; a.nq = nq; a.D = D;
            a.ptr = d_cp; a.items = d_ci; a.E = ncand; a.out = d_cs;
            CHECK(orx_launch_cand_score(c, a, k.kind));
            if (metrics) {
                a.ptr = d_pp; a.items = d_pi; a.E = npos; a.out = d_ps;
                CHECK(orx_launch_cand_score(c, a, k.kind));
            }
        }
        if (metrics) {
            CandRankArgs r;
            memset(&r, 0, sizeof(r));
            r.pos_ptr = d_pp; r.pos_items = d_pi; r.pos_s = d_ps; r.cand_ptr = d_cp; r.cand_items = d_ci; r.cand_s = d_cs;
            r.NB = k.NB; r.at = (const float*)(base + p.off[CD_AT]); r.nat = k.nat;
            r.auc = (float*)(base + p.off[CD_OUT]); r.ndcg = r.auc + nq; r.recall = r.ndcg + (size_t)nq * k.nat;
            CHECK(orx_launch_cand_rank(c, r, nq));
            CHECK(orx_fetch_metrics(c, r.auc, r.ndcg, r.recall, q0, nq, k.nat, k.auc, k.ndcg, k.recall));
        } else if (!k.scores_on_device && ncand) {
            ORX_HIP(hipMemcpyAsync(k.scores + cb, d_cs, (size_t)ncand * 4, hipMemcpyDeviceToHost, c->stream));
        }
        ORX_HIP(hipStreamSynchronize(c->stream));          // (the host staging vectors are refilled by the next batch)
        q0 += nq;
    }
    return dense ? orx_check_index_error(c) : ORX_OK;
}

extern "C" int orx_score_candidates(orx_ctx* c, int kind, orx_table* U, orx_table* V, orx_table* b, orx_table* w,
                                    const int32_t* uid, int64_t n, const int64_t* cand_ptr, const int32_t* cand_items, int flags,
                                    float* out) {
    static const char* fn = "orx_score_candidates";
    CHECK(orx_sync_tables({U, V, b, w}));
    ORX_ARG(cand_ptr || n == 0, "%s: NULL argument", fn);
    ORX_ARG((flags & ~ORX_OUT_DEVICE) == 0, "%s: unknown flags 0x%x", fn, flags);
    ORX_ARG(c && U && V && n >= 0 && (n == 0 || uid), "%s: NULL argument", fn);
    CHECK(orx_check_scorer(fn, c, kind, U, V, b, w, uid, n, true));
    if (n == 0) return ORX_OK;
    CHECK(orx_check_lists(fn, "candidate", cand_ptr, cand_items, n, V->rows, false, nullptr));
    if (cand_ptr[n] == 0) return ORX_OK;
    ORX_ARG(out, "%s: NULL output", fn);
    CandCall k;
    memset(&k, 0, sizeof(k));
    k.c = c; k.kind = kind; k.U = U; k.V = V; k.b = b; k.w = w; k.uid = uid; k.n = n;
    k.cand_ptr = cand_ptr; k.cand_items = cand_items; k.budget = ORX_CAND_SCRATCH;
    k.scores = out; k.scores_on_device = (flags & ORX_OUT_DEVICE) != 0;
    return cand_run(k);
}

extern "C" int orx_rank_metrics_candidates(orx_ctx* c, int kind, orx_table* U, orx_table* V, orx_table* b, orx_table* w,
                                           const int32_t* uid, int64_t n, const int64_t* pos_ptr, const int32_t* pos_items,
                                           const int64_t* cand_ptr, const int32_t* cand_items, const float* at, int32_t nat,
                                           size_t scratch_bytes, float* auc, float* ndcg, float* recall) {
    static const char* fn = "orx_rank_metrics_candidates";
    CHECK(orx_sync_tables({U, V, b, w}));
    ORX_ARG(pos_ptr && cand_ptr && at, "%s: NULL argument", fn);
    ORX_ARG(nat >= 1 && nat <= ORX_EVAL_NAT, "%s: nat must be in [1, 16]", fn);
    ORX_ARG(c && U && V && n >= 0 && (n == 0 || uid), "%s: NULL argument", fn);
    CHECK(orx_check_scorer(fn, c, kind, U, V, b, w, uid, n, true));
    if (n == 0) return ORX_OK;
    int64_t max_pos = 0, max_cand = 0;
    CHECK(orx_rank_metrics_candidates_check(n, V->rows, pos_ptr, pos_items, cand_ptr, cand_items, &max_pos, &max_cand));
    CandCall k;
    memset(&k, 0, sizeof(k));
    k.c = c; k.kind = kind; k.U = U; k.V = V; k.b = b; k.w = w; k.uid = uid; k.n = n;
    k.pos_ptr = pos_ptr; k.pos_items = pos_items; k.cand_ptr = cand_ptr; k.cand_items = cand_items;
    k.at = at; k.nat = nat; k.budget = scratch_bytes ? scratch_bytes : ORX_CAND_SCRATCH;
    k.NB = orx_rank_buckets(max_pos);                       // every user of every batch takes the call's chunking (rank_steps)
    k.auc = auc; k.ndcg = ndcg; k.recall = recall;
    return cand_run(k);
}
