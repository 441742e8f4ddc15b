// Diagnostic entry points of the duplicate plan of the exact steps: make the plan of K steps on the production route (orx_exact_buffers,
// orx_pairing_buffers, orx_plan_dedup_args, orx_exact_plan_issue / orx_exact_plan_finish for the bucketed plan of kernels_plan.hip,
// orx_launch_dedup / orx_launch_urgent for dedup_kernel + urgent_kernel) and hand every field of it back; and the geometry of the bucketed
// plan for a shape.  tests/test_gpu_plan.py holds each field to the contract its consumers rely on (tests/plan_ref.py).  The plan never
// touches a table: the tables here are stand-ins that carry a row count and a dim, so geometries of 2^27 rows and more cost no memory.
#include "orx_internal.h"

#include <cstring>
#include <vector>

extern "C" int orx_plan_geometry(int64_t NU, int64_t NI, int64_t nU, int64_t nP, int64_t nN, int32_t* out) {
    ORX_ARG(out && NU > 0 && NI > 0 && nU >= 0 && nP >= 0 && nN >= 0, "orx_plan_geometry: bad argument");
    DedupArgs d;
    memset(&d, 0, sizeof(d));
    d.nU = nU; d.nP = nP; d.nN = nN; d.NU = NU; d.NI = NI;
    orx_plan_geometry_query(d, out);
    out[14] = (int32_t)orx_dedup_range_rows(); out[15] = orx_dedup_buckets(NU);
    return ORX_OK;
}

namespace {
struct DevBuf {      // ids / labels of the call on the device, freed on every way out
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int put(const void* src, size_t bytes, hipStream_t st) {
        ORX_HIP(hipMalloc(&p, bytes < 16 ? 16 : bytes));
        ORX_HIP(hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, st));
        return ORX_OK;
    }
};
template <class T>
int fetch(std::vector<T>* h, const T* dev, size_t n, hipStream_t st) {
    h->resize(n);
    if (n) ORX_HIP(hipMemcpyAsync(h->data(), dev, n * sizeof(T), hipMemcpyDeviceToHost, st));
    return ORX_OK;
}
}  // namespace

// opts[8]: {plan version 1 / 2, staging, urgent marks (the in-launch apply), pairing tpw (0: off), min_late (-1: the heuristic),
//           force the 1024-thread workgroups, step0 (> 0: the chunk is planned as [0, step0) and [step0, K)), 0}
// out[10]: host buffers, each may be NULL: ids [K][3][B], pairing words [K][B], dlist [K][2B], dcount [K], alloc [K][8],
//          refinfo [K][3][B][2], segstart [K][B], dseg [K][2B], dcnt [K][2B], tree items [K][item_stride][4]
// info[8]: {item_stride, tree_off[0..2], index-error flag of the context (read, never cleared: orx_check_index_error still reports it), plan_big after the plan, Bp, steps per chunk}
// out == NULL: only the buffers are sized and info filled (a caller learns item_stride before it allocates).
extern "C" int orx_plan_dump(orx_ctx* c, const int32_t* uid, const int32_t* pid, const int32_t* nid, const float* label, int64_t K, int64_t B,
                             int64_t NU, int64_t NI, int32_t D, const int32_t* opts, void* const* out, int64_t* info) {
    ORX_ARG(c && opts && info && K > 0 && B > 0 && D > 0, "orx_plan_dump: bad argument");
    ORX_ARG(NU > 0 && NI > 0 && NU < (1LL << 28) && NI < (1LL << 28), "orx_plan_dump: the rewritten ids carry role and urgent bits: tables below 2^28 rows");
    const int version = opts[0], tpw = opts[3], min_late = opts[4];
    const bool staging = opts[1] != 0, inline_apply = opts[2] != 0, force_big = opts[5] != 0;
    const int64_t step0 = opts[6];
    ORX_ARG(version == 1 || version == 2, "orx_plan_dump: plan version 1 or 2");
    ORX_ARG((version == 2) == orx_plan_v2(true), "orx_plan_dump: plan version %d asked for, the process runs the other one (ORX_PLAN_V1 is read once)", version);
    ORX_ARG(tpw == 0 || (version == 2 && tpw == orx_fused_tpw(D) && tpw > 1 && B >= 2), "orx_plan_dump: pairing needs the bucketed plan and tpw = orx_fused_tpw(D) > 1");
    ORX_ARG(step0 >= 0 && step0 < K && (step0 == 0 || version == 2), "orx_plan_dump: 0 <= step0 < K, bucketed plan only");
    ORX_ARG(!label || (nid == nullptr), "orx_plan_dump: labels belong to a pointwise step (no nid)");
    ORX_ARG(out == nullptr || (uid && pid), "orx_plan_dump: NULL ids");
    ORX_ARG(out == nullptr || tpw == 0 || nid || label, "orx_plan_dump: the input records of a pointwise step with pairing carry the labels");
    ORX_HIP(hipSetDevice(c->device));
    const int64_t nN = nid ? B : 0;
    orx_table U, V;
    U.ctx = V.ctx = c; U.rows = NU; V.rows = NI; U.dim = V.dim = D; U.owned = V.owned = false;
    PairPlan plan;
    CHECK(orx_exact_buffers(c, &U, &V, K, B, MODE_EXACT, true, inline_apply, staging, orx_dedup_buckets(NU) + orx_dedup_buckets(NI), orx_fused_nwaves(D, B), &plan));
    ORX_ARG(K <= plan.chunk, "orx_plan_dump: %lld steps, a chunk of this batch size holds %lld", (long long)K, (long long)plan.chunk);
    if (tpw) CHECK(orx_pairing_buffers(c, B, D, &plan));
    plan.min_late = min_late;
    info[0] = plan.item_stride; info[1] = plan.tree_off[0]; info[2] = plan.tree_off[1]; info[3] = plan.tree_off[2];
    info[4] = 0; info[5] = c->plan_big; info[6] = plan.Bp; info[7] = plan.chunk;
    if (out == nullptr) return ORX_OK;

    DevBuf du, dp, dn, dl;
    const size_t idb = (size_t)K * B * sizeof(int32_t);
    CHECK(du.put(uid, idb, c->stream)); CHECK(dp.put(pid, idb, c->stream));
    if (nid) CHECK(dn.put(nid, idb, c->stream));
    if (label) CHECK(dl.put(label, idb, c->stream));
    const int32_t *u = (const int32_t*)du.p, *p = (const int32_t*)dp.p, *n = (const int32_t*)dn.p;
    if (version == 2) {
        c->plan_label = (const float*)dl.p;
        const int pause = c->pair_pause;      // (a diagnostic plan does not decide whether the next train call pairs)
        int rc = ORX_OK;
        const int64_t lo[2] = {0, step0}, cnt[2] = {step0 ? step0 : K, step0 ? K - step0 : 0};
        for (int piece = 0; piece < 2 && rc == ORX_OK && cnt[piece] > 0; ++piece) {
            if (force_big) c->plan_big = true;
            ExactChunk ck;
            rc = orx_exact_plan_issue(c, &U, &V, u + lo[piece] * B, p + lo[piece] * B, n ? n + lo[piece] * B : nullptr, B, B, B, nN, cnt[piece], B,
                                      inline_apply, staging, plan, lo[piece], c->plan_ev, nullptr);
            if (rc == ORX_OK) rc = orx_exact_plan_finish(c, cnt[piece], B, inline_apply, staging, lo[piece], c->plan_ev, &ck, tpw > 1);
        }
        c->plan_label = nullptr;
        c->pair_pause = pause;
        CHECK(rc);
    } else {
        DedupArgs d;
        orx_plan_dedup_args(c, &U, &V, u, p, n, B, B, B, nN, B, true, inline_apply, staging, plan, 0, &d);
        ORX_HIP(hipMemsetAsync(c->d_dcount, 0, (size_t)K * sizeof(int), c->stream));
        if (staging) {
            ORX_HIP(hipMemsetAsync(c->d_tricnt, 0, (size_t)K * B * sizeof(int), c->stream));
            ORX_HIP(hipMemsetAsync(c->d_alloc, 0, (size_t)K * 8 * sizeof(int), c->stream));
        }
        CHECK(orx_launch_dedup(c, d, K));
        if (inline_apply) CHECK(orx_launch_urgent(c, d, K));
    }
    info[5] = c->plan_big;

    // everything the plan wrote, per step and with the padding between the three id arrays of a step removed
    const int64_t Bp = plan.Bp, ls = plan.list_stride;
    hipStream_t st = c->stream;
    std::vector<int32_t> h_ids; std::vector<int4> h_ids4; std::vector<uint32_t> h_dlist; std::vector<int> h_dcount, h_alloc, h_seg, h_dseg, h_dcnt;
    std::vector<int2> h_ref; std::vector<int4> h_items;
    int flag = 0;
    if (tpw) CHECK(fetch(&h_ids4, (const int4*)c->d_ids4, (size_t)K * B, st));
    else CHECK(fetch(&h_ids, (const int32_t*)c->d_ids2, (size_t)K * 3 * Bp, st));
    CHECK(fetch(&h_dlist, (const uint32_t*)c->d_dlist, (size_t)K * ls, st));
    CHECK(fetch(&h_dcount, (const int*)c->d_dcount, (size_t)K, st));
    if (version == 2 || staging) CHECK(fetch(&h_alloc, (const int*)c->d_alloc, (size_t)K * 8, st));
    if (staging) {
        CHECK(fetch(&h_ref, (const int2*)c->d_refinfo, (size_t)K * 3 * Bp, st));
        CHECK(fetch(&h_seg, (const int*)c->d_segstart, (size_t)K * B, st));
        CHECK(fetch(&h_dseg, (const int*)c->d_dseg, (size_t)K * ls, st));
        CHECK(fetch(&h_dcnt, (const int*)c->d_dcnt, (size_t)K * ls, st));
        CHECK(fetch(&h_items, (const int4*)c->d_chunks, (size_t)K * plan.item_stride, st));
    }
    ORX_HIP(hipMemcpyAsync(&flag, c->d_err, sizeof(int), hipMemcpyDeviceToHost, st));
    ORX_HIP(hipStreamSynchronize(st));
    info[4] = flag;
    const int nslot = nid ? 3 : 2;
    if (out[0]) {
        int32_t* o = (int32_t*)out[0];
        for (int64_t s = 0; s < K; ++s)
            for (int k = 0; k < 3; ++k)
                for (int64_t j = 0; j < B; ++j) {
                    int32_t v = 0;
                    if (tpw) { const int4 r = h_ids4[(size_t)s * B + j]; v = k == 0 ? r.x : (k == 1 ? r.y : r.z); }
                    else if (k < nslot) v = h_ids[(size_t)s * 3 * Bp + (size_t)k * Bp + j];
                    o[((size_t)s * 3 + k) * B + j] = v;
                }
    }
    if (out[1]) {
        int32_t* o = (int32_t*)out[1];
        for (size_t i = 0; i < (size_t)K * B; ++i) o[i] = tpw ? h_ids4[i].w : (int32_t)((uint32_t)(i % (size_t)B) << 10);
    }
    if (out[2]) memcpy(out[2], h_dlist.data(), h_dlist.size() * sizeof(uint32_t));
    if (out[3]) memcpy(out[3], h_dcount.data(), h_dcount.size() * sizeof(int));
    if (out[4]) { if (h_alloc.empty()) memset(out[4], 0, (size_t)K * 8 * sizeof(int)); else memcpy(out[4], h_alloc.data(), h_alloc.size() * sizeof(int)); }
    if (staging) {
        if (out[5]) {
            int32_t* o = (int32_t*)out[5];
            for (int64_t s = 0; s < K; ++s)
                for (int k = 0; k < 3; ++k)
                    for (int64_t j = 0; j < B; ++j) {
                        const int2 r = k < nslot ? h_ref[(size_t)s * 3 * Bp + (size_t)k * Bp + j] : make_int2(0, 0);
                        o[(((size_t)s * 3 + k) * B + j) * 2] = r.x; o[(((size_t)s * 3 + k) * B + j) * 2 + 1] = r.y;
                    }
        }
        if (out[6]) memcpy(out[6], h_seg.data(), h_seg.size() * sizeof(int));
        if (out[7]) memcpy(out[7], h_dseg.data(), h_dseg.size() * sizeof(int));
        if (out[8]) memcpy(out[8], h_dcnt.data(), h_dcnt.size() * sizeof(int));
        if (out[9]) memcpy(out[9], h_items.data(), h_items.size() * sizeof(int4));
    }
    return ORX_OK;
}
