// C-ABI entry points of the candidate lists: orx_score_candidates, orx_rank_metrics_candidates and the host-only list check
// (kernels_cand.hip has the semantics and the design).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orx_internal.h"

static constexpr size_t ORX_CAND_SCRATCH = (size_t)512 << 20;       // default budget of one batch of users
static constexpr int64_t ORX_CAND_MAX_DENSE_BATCH = 32768;          // (users are a grid dimension of the scorer)
static constexpr int ORX_CAND_NAT = 16;

static size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- argument checks, all on the host ---------------------------------------------------------------------------------
static int cand_check_list(const char* fn, const char* what, const int64_t* ptr, const int32_t* items, int64_t n, int64_t NI,
                           bool ascending, int64_t* longest) {
    ORX_ARG(ptr[0] == 0, "%s: the %s lists start at offset 0", fn, what);
    *longest = 0;
    for (int64_t q = 0; q < n; ++q) {
        ORX_ARG(ptr[q + 1] >= ptr[q], "%s: %s offsets must not decrease", fn, what);
        *longest = std::max(*longest, ptr[q + 1] - ptr[q]);
    }
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

extern "C" int orx_rank_metrics_candidates_check(int64_t n, int64_t items, const int64_t* pos_ptr, const int32_t* pos_items,
                                                 const int64_t* cand_ptr, const int32_t* cand_items, int64_t* max_pos,
                                                 int64_t* max_cand) {
    static const char* fn = "orx_rank_metrics_candidates";
    ORX_ARG(pos_ptr && cand_ptr && max_pos && max_cand && n >= 0 && items > 0, "%s: NULL argument", fn);
    *max_pos = 0; *max_cand = 0;
    if (n == 0) return ORX_OK;
    CHECK(cand_check_list(fn, "positive", pos_ptr, pos_items, n, items, true, max_pos));
    return cand_check_list(fn, "candidate", cand_ptr, cand_items, n, items, true, max_cand);
}

static int cand_check_tables(const char* fn, orx_ctx* c, int kind, orx_table* U, orx_table* V, orx_table* b, orx_table* w,
                             const int32_t* uid, int64_t n) {
    ORX_ARG(c && U && V && n >= 0 && (n == 0 || uid), "%s: NULL argument", fn);
    ORX_ARG(kind >= 0 && kind <= 2 && U->dim == V->dim && U->dim <= 1024, "%s: bad scorer arguments", fn);
    ORX_ARG(!b || (b->rows == V->rows && b->dim == 1), "%s: table shapes do not match", fn);
    ORX_ARG(kind != 2 || (w && w->rows == U->dim && w->dim == 1), "%s: GMF needs w [D, 1]", fn);
    for (int64_t q = 0; q < n; ++q) {
        if (uid[q] < 0 || uid[q] >= U->rows) {
            orx_set_error("%s: user id %d outside [0, %lld)", fn, uid[q], (long long)U->rows);
            return ORX_ERR_INDEX;
        }
    }
    return ORX_OK;
}

// ---- the batches both entry points share ----------------------------------------------------------------------------------
// pieces of d_dflag of one batch
enum { CD_AT, CD_UID, CD_PP, CD_CP, CD_PI, CD_CI, CD_PS, CD_CS, CD_OUT, CD_PIECES };

struct CandBatch {
    size_t off[CD_PIECES];
    size_t list_bytes;          // d_dflag
    int64_t rows;               // dense route: score rows (at least 65 when the call has more than 64 users: the scorer's 128-user tile)
    size_t bytes;               // all of it
};

static void cand_sizes(CandBatch* p, bool dense, int64_t n, int64_t nq, int64_t npos, int64_t ncand, int64_t items) {
    const size_t u = (size_t)nq;
    const size_t sz[CD_PIECES] = {64, u * 4, (u + 1) * 8, (u + 1) * 8, (size_t)npos * 4, (size_t)ncand * 4, (size_t)npos * 4,
                                  (size_t)ncand * 4, u * (1 + 2 * ORX_CAND_NAT) * 4};
    size_t total = 0;
    for (int i = 0; i < CD_PIECES; ++i) { p->off[i] = total; total += al256(sz[i]); }
    p->list_bytes = total;
    p->rows = dense ? (n > 64 ? std::max<int64_t>(nq, 65) : nq) : 0;
    p->bytes = total + (size_t)p->rows * items * 4 + (size_t)p->rows * 4;
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
    static thread_local std::vector<int32_t> huid;
    static thread_local std::vector<float> hout;
    float hat[16] = {0};
    if (metrics) memcpy(hat, k.at, sizeof(float) * k.nat);
    const float* Ub = k.U->w; const float* Vb = k.V->w;
    const float* bb = k.b ? k.b->w : nullptr; const float* wb = k.w ? k.w->w : nullptr;
    for (int64_t q0 = 0; q0 < n;) {
        // the longest run of users whose lists, scores and (dense route) score rows stay within the budget; one user at least
        CandBatch p;
        int64_t nq = 1;
        auto sizes = [&](int64_t m) {
            cand_sizes(&p, dense, n, m, metrics ? k.pos_ptr[q0 + m] - k.pos_ptr[q0] : 0, k.cand_ptr[q0 + m] - k.cand_ptr[q0], NI);
        };
        {
            int64_t lo = 1, hi = n - q0;
            if (dense) hi = std::min(hi, ORX_CAND_MAX_DENSE_BATCH);
            while (lo < hi) {                              // (the sizes grow with the run)
                const int64_t mid = (lo + hi + 1) / 2;
                sizes(mid);
                if (p.bytes <= k.budget) lo = mid; else hi = mid - 1;
            }
            nq = lo;
            sizes(nq);
        }
        const int64_t pb = metrics ? k.pos_ptr[q0] : 0, cb = k.cand_ptr[q0];
        const int64_t npos = metrics ? k.pos_ptr[q0 + nq] - pb : 0, ncand = k.cand_ptr[q0 + nq] - cb;
        ENSURE(c->d_dflag, c->d_dflag_cap, p.list_bytes);
        unsigned char* base = c->d_dflag;
        int32_t* d_uid = (int32_t*)(base + p.off[CD_UID]);
        int64_t* d_pp = (int64_t*)(base + p.off[CD_PP]); int64_t* d_cp = (int64_t*)(base + p.off[CD_CP]);
        int32_t* d_pi = (int32_t*)(base + p.off[CD_PI]); int32_t* d_ci = (int32_t*)(base + p.off[CD_CI]);
        float* d_ps = (float*)(base + p.off[CD_PS]);
        float* d_cs = (!metrics && k.scores_on_device) ? k.scores + cb : (float*)(base + p.off[CD_CS]);
        hp.resize(2 * (nq + 1));
        for (int64_t q = 0; q <= nq; ++q) { hp[q] = metrics ? k.pos_ptr[q0 + q] - pb : 0; hp[nq + 1 + q] = k.cand_ptr[q0 + q] - cb; }
        ORX_HIP(hipMemcpyAsync(d_uid, k.uid + q0, (size_t)nq * 4, hipMemcpyHostToDevice, c->stream));
        ORX_HIP(hipMemcpyAsync(d_cp, hp.data() + nq + 1, (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, c->stream));
        if (ncand) ORX_HIP(hipMemcpyAsync(d_ci, k.cand_items + cb, (size_t)ncand * 4, hipMemcpyHostToDevice, c->stream));
        if (metrics) {
            ORX_HIP(hipMemcpyAsync(base + p.off[CD_AT], hat, 64, hipMemcpyHostToDevice, c->stream));
            ORX_HIP(hipMemcpyAsync(d_pp, hp.data(), (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, c->stream));
            if (npos) ORX_HIP(hipMemcpyAsync(d_pi, k.pos_items + pb, (size_t)npos * 4, hipMemcpyHostToDevice, c->stream));
        }
        if (dense) {
            if (npos + ncand > 0) {
                ENSURE(c->d_tmp, c->d_tmp_cap, (size_t)p.rows * NI * 4);
                ENSURE(c->d_ids, c->d_ids_cap, (size_t)p.rows * 4);
                huid.assign(k.uid + q0, k.uid + q0 + nq);
                huid.resize(p.rows, k.uid[q0]);           // rows beyond the batch: the scorer's wide tile, their scores are never read
                CHECK(stage_ids(c, huid.data(), p.rows, 0));
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
            if (k.auc) ORX_HIP(hipMemcpyAsync(k.auc + q0, r.auc, sizeof(float) * nq, hipMemcpyDeviceToHost, c->stream));
            if (k.ndcg) ORX_HIP(hipMemcpyAsync(k.ndcg + (size_t)q0 * k.nat, r.ndcg, sizeof(float) * nq * k.nat, hipMemcpyDeviceToHost, c->stream));
            if (k.recall) ORX_HIP(hipMemcpyAsync(k.recall + (size_t)q0 * k.nat, r.recall, sizeof(float) * nq * k.nat, hipMemcpyDeviceToHost, c->stream));
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
    if (U) CHECK(orx_table_sync(U));
    if (V) CHECK(orx_table_sync(V));
    if (b) CHECK(orx_table_sync(b));
    if (w) CHECK(orx_table_sync(w));
    ORX_ARG(cand_ptr || n == 0, "%s: NULL argument", fn);
    ORX_ARG((flags & ~ORX_OUT_DEVICE) == 0, "%s: unknown flags 0x%x", fn, flags);
    CHECK(cand_check_tables(fn, c, kind, U, V, b, w, uid, n));
    if (n == 0) return ORX_OK;
    int64_t longest = 0;
    CHECK(cand_check_list(fn, "candidate", cand_ptr, cand_items, n, V->rows, false, &longest));
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
    if (U) CHECK(orx_table_sync(U));
    if (V) CHECK(orx_table_sync(V));
    if (b) CHECK(orx_table_sync(b));
    if (w) CHECK(orx_table_sync(w));
    ORX_ARG(pos_ptr && cand_ptr && at, "%s: NULL argument", fn);
    ORX_ARG(nat >= 1 && nat <= ORX_CAND_NAT, "%s: nat must be in [1, 16]", fn);
    CHECK(cand_check_tables(fn, c, kind, U, V, b, w, uid, n));
    if (n == 0) return ORX_OK;
    int64_t max_pos = 0, max_cand = 0;
    CHECK(orx_rank_metrics_candidates_check(n, V->rows, pos_ptr, pos_items, cand_ptr, cand_items, &max_pos, &max_cand));
    CandCall k;
    memset(&k, 0, sizeof(k));
    k.c = c; k.kind = kind; k.U = U; k.V = V; k.b = b; k.w = w; k.uid = uid; k.n = n;
    k.pos_ptr = pos_ptr; k.pos_items = pos_items; k.cand_ptr = cand_ptr; k.cand_items = cand_items;
    k.at = at; k.nat = nat; k.budget = scratch_bytes ? scratch_bytes : ORX_CAND_SCRATCH;
    k.NB = max_pos <= 7 ? 8 : (max_pos <= 15 ? 16 : 64);    // every user of every batch takes the call's chunking (rank_steps)
    k.auc = auc; k.ndcg = ndcg; k.recall = recall;
    return cand_run(k);
}
