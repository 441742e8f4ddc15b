// Weighted item proposal of the sampler's negatives: the host-only alias-table builder (orx_alias_build) and the table a sampler
// keeps on the device (orx_sampler_set_proposal, orx_sampler_proposal_read).  include/openrec_hip.h has the contract; the draw
// itself is in kernels_sampler.hip / kernels_hardneg.hip.
#include <climits>
#include <cmath>

#include "orx_internal.h"

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
    if (!s->d_prop) ORX_HIP(hipMalloc((void**)&s->d_prop, sizeof(uint2) * n));
    ORX_HIP(hipStreamSynchronize(s->ctx->stream));            // draws enqueued before this call read the old table
    ORX_HIP(hipMemcpy(s->d_prop, rec.data(), sizeof(uint2) * n, hipMemcpyHostToDevice));
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
