// C-ABI entry points of the top-K recommendation: orx_recommend_topk (scores never stored, kernels_topk.hip has the
// semantics and the design) and orx_topk_rows (the same selection over scores that exist already).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orx_internal.h"

static constexpr size_t ORX_TOPK_DENSE_BYTES = (size_t)256 << 20;   // dense score rows (direct route, fallback, host rows)
static constexpr size_t ORX_TOPK_BATCH_BYTES = (size_t)512 << 20;   // sample rows + candidate lists of one batch of users
static constexpr int ORX_TOPK_MAX_K = 1024;

// device scratch of one batch of nb users (d_topk), 256-byte aligned pieces
struct TopkScratch {
    float* theta; int* cnt; float* cs; int32_t* ci;
    int64_t* eptr; int32_t* eitems; int32_t* rowmap; int32_t* uidsub;
    int32_t* oi; float* os;
    int2* pool_iu; float* pool_s;           // the filter's per-workgroup candidate pools (fused route only)
};

static int topk_scratch(orx_ctx* c, int64_t nb, int C, int64_t max_excl, int k, TopkScratch* s) {
    const size_t pool = C ? (size_t)TOPK_FILTER_BLOCKS * TOPK_POOL : 0;
    const size_t sizes[12] = {(size_t)nb * 4, (size_t)nb * 4, (size_t)nb * C * 4, (size_t)nb * C * 4, (size_t)(nb + 1) * 8,
                              (size_t)max_excl * 4, (size_t)nb * 4, (size_t)nb * 4, (size_t)nb * k * 4, (size_t)nb * k * 4,
                              pool * 8, pool * 4};
    size_t off[12];
    ENSURE(c->d_topk, c->d_topk_cap, orx_layout(sizes, 12, off));
    unsigned char* p = c->d_topk;
    s->theta = (float*)(p + off[0]); s->cnt = (int*)(p + off[1]); s->cs = (float*)(p + off[2]); s->ci = (int32_t*)(p + off[3]);
    s->eptr = (int64_t*)(p + off[4]); s->eitems = (int32_t*)(p + off[5]); s->rowmap = (int32_t*)(p + off[6]);
    s->uidsub = (int32_t*)(p + off[7]); s->oi = (int32_t*)(p + off[8]); s->os = (float*)(p + off[9]);
    s->pool_iu = (int2*)(p + off[10]); s->pool_s = (float*)(p + off[11]);
    return ORX_OK;
}

static int64_t topk_max_excl(const int64_t* ptr, int64_t n, int64_t nb) {
    int64_t m = 0;
    if (ptr) for (int64_t q0 = 0; q0 < n; q0 += nb) m = std::max(m, ptr[std::min(n, q0 + nb)] - ptr[q0]);
    return m;
}

// the exclusion rows of users [q0, q0 + nq) to the device, rebased to 0 and sorted inside each row (the kernels search them)
static int topk_stage_excl(orx_ctx* c, const int64_t* ptr, const int32_t* items, int64_t q0, int64_t nq, const TopkScratch& s,
                           std::vector<int64_t>& hp, std::vector<int32_t>& hi) {
    hp.resize(nq + 1);
    return orx_stage_csr(c, ptr, items, q0, nq, hp.data(), &hi, s.eptr, s.eitems, nullptr);
}

// the given batch users scored densely, a bounded number of rows at a time, and selected: the direct route and the fallback.
// wide: the call has more than 64 users, and so does every scorer launch here where there are that many rows (orx_dense_rows)
static int topk_dense_users(orx_ctx* c, int kind, orx_table* U, orx_table* V, orx_table* b, orx_table* w, const int32_t* huid,
                            const std::vector<int32_t>& local, const TopkScratch& s, bool excl, bool wide, int k, int32_t* oi,
                            float* os, std::vector<int32_t>& huid_sub) {
    const int64_t NI = V->rows, nl = (int64_t)local.size();
    if (nl == 0) return ORX_OK;
    int64_t per = std::max<int64_t>(1, std::min<int64_t>(nl, (int64_t)(ORX_TOPK_DENSE_BYTES / ((size_t)NI * 4))));
    if (wide && nl > 64) per = std::max<int64_t>(per, 65);
    const int64_t nbatch = std::max<int64_t>(1, nl / per);          // nbatch groups of per .. 2 per - 1 rows
    ENSURE(c->d_tmp, c->d_tmp_cap, (size_t)((nl + nbatch - 1) / nbatch) * NI * sizeof(float));
    huid_sub.resize(nl);
    for (int64_t i = 0; i < nl; ++i) huid_sub[i] = huid[local[i]];
    ORX_HIP(hipMemcpyAsync(s.rowmap, local.data(), (size_t)nl * 4, hipMemcpyHostToDevice, c->stream));
    ORX_HIP(hipMemcpyAsync(s.uidsub, huid_sub.data(), (size_t)nl * 4, hipMemcpyHostToDevice, c->stream));
    for (int64_t bi = 0; bi < nbatch; ++bi) {
        const int64_t i0 = bi * nl / nbatch, nr = (bi + 1) * nl / nbatch - i0;
        CHECK(orx_launch_score_all(c, U->w, V->w, b ? b->w : nullptr, w ? w->w : nullptr, s.uidsub + i0, nr, U->rows, NI, U->dim,
                                   kind, c->d_tmp));
        TopkSelectArgs a;
        memset(&a, 0, sizeof(a));
        a.scores = c->d_tmp; a.ld = NI; a.m = NI; a.rowmap = s.rowmap + i0;
        a.eptr = excl ? s.eptr : nullptr; a.eitems = s.eitems; a.k = k; a.out_items = oi; a.out_scores = os;
        CHECK(orx_launch_topk_select(c, a, nr));
    }
    return ORX_OK;
}

extern "C" int orx_recommend_topk(orx_ctx* c, int kind, orx_table* U, orx_table* V, orx_table* b, orx_table* w,
                                  const int32_t* uid, int64_t n, const int64_t* excl_ptr, const int32_t* excl_items, int32_t k,
                                  int flags, int32_t* out_items, float* out_scores) {
    static const char* fn = "orx_recommend_topk";
    CHECK(orx_sync_tables({U, V, b, w}));
    ORX_ARG(c && U && V && n >= 0 && (n == 0 || (uid && out_items && out_scores)), "%s: NULL argument", fn);
    ORX_ARG(k >= 1 && k <= ORX_TOPK_MAX_K, "%s: k = %d outside [1, %d]", fn, k, ORX_TOPK_MAX_K);
    ORX_ARG((flags & ~ORX_OUT_DEVICE) == 0, "%s: unknown flags 0x%x", fn, flags);
    CHECK(orx_check_scorer(fn, c, kind, U, V, b, w, uid, n, true));
    if (excl_ptr) CHECK(orx_check_lists(fn, "exclusion", excl_ptr, excl_items, n, V->rows, false, nullptr));
    if (n == 0) return ORX_OK;
    ORX_HIP(hipSetDevice(c->device));
    const int64_t NI = V->rows;
    const int D = U->dim;
    const bool dev_out = (flags & ORX_OUT_DEVICE) != 0;
    // candidate capacity C and sample size P: the sample's k-th best leaves about k NI / P candidates, an eighth of C
    int C = 8192;
    while (C < 160 * k && C < 65536) C <<= 1;
    int64_t P = std::max<int64_t>(8192, (8 * (int64_t)k * NI + C - 1) / C);
    P = (P + 63) / 64 * 64;
    const bool fused = kind != 1 && D <= 256 && getenv("ORX_SCORE_SIMPLE") == nullptr && P < NI;     // (kernels_topk.hip: why not L2)
    const size_t per_user = fused ? (size_t)P * 4 + (size_t)C * 8 + 16 + (size_t)k * 8 : 16 + (size_t)k * 8;
    const int64_t nbmax = fused ? std::max<int64_t>(64, std::min<int64_t>(4096, (int64_t)(ORX_TOPK_BATCH_BYTES / per_user))) : 4096;
    const int64_t nbatch = (n + nbmax - 1) / nbmax, nb = (n + nbatch - 1) / nbatch;
    TopkScratch s;
    CHECK(topk_scratch(c, nb, fused ? C : 0, topk_max_excl(excl_ptr, n, nb), k, &s));
    ENSURE(c->d_ids, c->d_ids_cap, (size_t)nb * sizeof(int32_t));
    if (fused) ENSURE(c->d_tmp, c->d_tmp_cap, (size_t)nb * P * sizeof(float));
    static thread_local std::vector<int64_t> hp;
    static thread_local std::vector<int32_t> hi, local, huid_sub;
    static thread_local std::vector<int> hcnt;
    for (int64_t q0 = 0; q0 < n; q0 += nb) {
        const int64_t nq = std::min(nb, n - q0);
        int32_t* oi = dev_out ? out_items + q0 * k : s.oi;
        float* os = dev_out ? out_scores + q0 * k : s.os;
        CHECK(stage_ids(c, uid + q0, nq, 0));
        if (excl_ptr) CHECK(topk_stage_excl(c, excl_ptr, excl_items, q0, nq, s, hp, hi));
        local.clear();
        if (fused) {
            // 1. thresholds from the first P items
            CHECK(orx_launch_score_all(c, U->w, V->w, b ? b->w : nullptr, w ? w->w : nullptr, c->d_ids, nq, U->rows, P, D, kind, c->d_tmp));
            TopkSelectArgs a;
            memset(&a, 0, sizeof(a));
            a.scores = c->d_tmp; a.ld = P; a.m = P; a.eptr = excl_ptr ? s.eptr : nullptr; a.eitems = s.eitems; a.k = k;
            a.theta = s.theta; a.cnt = s.cnt; a.C = C;
            CHECK(orx_launch_topk_select(c, a, nq));
            // 2. every item scored, the candidates kept
            bool launched = false;
            CHECK(orx_launch_topk_filter(c, U->w, V->w, b ? b->w : nullptr, w ? w->w : nullptr, c->d_ids, nq, U->rows, NI, D, kind,
                                         s.theta, s.cnt, s.cs, s.ci, C, s.pool_iu, s.pool_s, &launched));
            ORX_ARG(launched, "orx_recommend_topk: no MFMA tile for dim %d", D);
            // 3. selection over the candidates, the excluded ones left out
            memset(&a, 0, sizeof(a));
            a.cs = s.cs; a.ci = s.ci; a.cnt = s.cnt; a.C = C; a.k = k; a.out_items = oi; a.out_scores = os;
            a.eptr = excl_ptr ? s.eptr : nullptr; a.eitems = s.eitems;
            CHECK(orx_launch_topk_select(c, a, nq));
            // 4. the users whose candidates overflowed, densely
            hcnt.resize(nq);
            ORX_HIP(hipMemcpyAsync(hcnt.data(), s.cnt, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, c->stream));
            ORX_HIP(hipStreamSynchronize(c->stream));
            for (int64_t q = 0; q < nq; ++q) if (hcnt[q] > C) local.push_back((int32_t)q);
        } else {
            for (int64_t q = 0; q < nq; ++q) local.push_back((int32_t)q);
        }
        CHECK(topk_dense_users(c, kind, U, V, b, w, uid + q0, local, s, excl_ptr != nullptr, n > 64, k, oi, os, huid_sub));
        if (!dev_out) {
            ORX_HIP(hipMemcpyAsync(out_items + q0 * k, oi, (size_t)nq * k * 4, hipMemcpyDeviceToHost, c->stream));
            ORX_HIP(hipMemcpyAsync(out_scores + q0 * k, os, (size_t)nq * k * 4, hipMemcpyDeviceToHost, c->stream));
        }
        ORX_HIP(hipStreamSynchronize(c->stream));          // (the host staging vectors are refilled by the next batch)
    }
    return orx_check_index_error(c);
}

extern "C" int orx_topk_rows(orx_ctx* c, const float* scores, int32_t scores_on_device, int64_t n, int64_t m,
                             const int64_t* excl_ptr, const int32_t* excl_items, int32_t k, int32_t* out_items, float* out_scores) {
    ORX_ARG(c && n >= 0 && m >= 1 && (n == 0 || (scores && out_items && out_scores)), "orx_topk_rows: NULL argument");
    ORX_ARG(k >= 1 && k <= ORX_TOPK_MAX_K, "orx_topk_rows: k = %d outside [1, %d]", k, ORX_TOPK_MAX_K);
    if (excl_ptr) CHECK(orx_check_lists("orx_topk_rows", "exclusion", excl_ptr, excl_items, n, m, false, nullptr));
    if (n == 0) return ORX_OK;
    ORX_HIP(hipSetDevice(c->device));
    const int64_t nb = scores_on_device ? std::min<int64_t>(n, 4096)
                                        : std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)(ORX_TOPK_DENSE_BYTES / ((size_t)m * 4))));
    TopkScratch s;
    CHECK(topk_scratch(c, nb, 0, topk_max_excl(excl_ptr, n, nb), k, &s));
    if (!scores_on_device) ENSURE(c->d_tmp, c->d_tmp_cap, (size_t)nb * m * sizeof(float));
    static thread_local std::vector<int64_t> hp;
    static thread_local std::vector<int32_t> hi;
    for (int64_t q0 = 0; q0 < n; q0 += nb) {
        const int64_t nq = std::min(nb, n - q0);
        if (excl_ptr) CHECK(topk_stage_excl(c, excl_ptr, excl_items, q0, nq, s, hp, hi));
        const float* rows = scores + (size_t)q0 * m;
        if (!scores_on_device) {
            ORX_HIP(hipMemcpyAsync(c->d_tmp, rows, (size_t)nq * m * sizeof(float), hipMemcpyHostToDevice, c->stream));
            rows = c->d_tmp;
        }
        TopkSelectArgs a;
        memset(&a, 0, sizeof(a));
        a.scores = rows; a.ld = m; a.m = m; a.eptr = excl_ptr ? s.eptr : nullptr; a.eitems = s.eitems; a.k = k;
        a.out_items = s.oi; a.out_scores = s.os;
        CHECK(orx_launch_topk_select(c, a, nq));
        ORX_HIP(hipMemcpyAsync(out_items + q0 * k, s.oi, (size_t)nq * k * 4, hipMemcpyDeviceToHost, c->stream));
        ORX_HIP(hipMemcpyAsync(out_scores + q0 * k, s.os, (size_t)nq * k * 4, hipMemcpyDeviceToHost, c->stream));
        ORX_HIP(hipStreamSynchronize(c->stream));
    }
    return ORX_OK;
}
