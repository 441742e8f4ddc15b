// The segment plan of the calls that cut the long rows of a CSR into segments of SEG entries (kernels_als.hip, kernels_graph.hip;
// api_csr.hip carves the scratch).  One thread per row of the call: a row of more than SEG entries takes nseg consecutive scratch
// slots (an INTEGER counter: the slot NUMBERS depend on the launch, what a consumer writes into a slot does not) and lists its
// segments; a row that does not fit into the `cap` slots any more gets none and is walked by its own consumer alone.
#pragma once
#include "orx_internal.h"

struct SegScratch { int cap; unsigned long long* counter; int* seg_base; int2* list; float* slots; };      // what the host carved (cap 0: no plan)
struct SegPlan { const int* seg_base; const int2* list; const unsigned long long* counter; int cap; float* slots; };      // what the consumers read

template <int SEG>
__global__ __launch_bounds__(256) void seg_plan_kernel(const int64_t* __restrict__ rp, int64_t nrows, int cap, unsigned long long* __restrict__ counter,
                                                       int* __restrict__ seg_base, int2* __restrict__ list) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrows) return;
    const int64_t n = rp[i + 1] - rp[i];
    int base = -1;
    if (n > SEG) {
        const int64_t nseg64 = (n + SEG - 1) / SEG;
        if (nseg64 <= cap) {
            const int nseg = (int)nseg64;
            const unsigned long long got = atomicAdd(counter, (unsigned long long)nseg);      // 64 bits: it never wraps
            if (got + nseg <= (unsigned long long)cap) {
                base = (int)got;
                for (int sg = 0; sg < nseg; ++sg) list[base + sg] = make_int2((int)i, sg);
            } else if (got < (unsigned long long)cap) {
                for (int sg = (int)got; sg < cap; ++sg) list[sg] = make_int2(-1, -1);      // slots nobody uses
            }
        }
    }
    seg_base[i] = base;
}

// how many entries of the list a segment kernel walks
__device__ __forceinline__ int seg_plan_count(const SegPlan& p) {
    const unsigned long long used = *p.counter;
    return used < (unsigned long long)p.cap ? (int)used : p.cap;
}

// the plan on the context's stream (cap 0: nothing, and no row looks for a slot) -> what the consumers read
template <int SEG>
int seg_plan_launch(orx_ctx* ctx, const int64_t* rp, int64_t nrows, const SegScratch& s, SegPlan* out) {
    const bool plan = s.cap > 0;
    *out = SegPlan{plan ? s.seg_base : nullptr, s.list, s.counter, s.cap, s.slots};
    if (plan) {
        ORX_HIP(hipMemsetAsync(s.counter, 0, sizeof(unsigned long long), ctx->stream));
        ORX_LAUNCH(ctx, seg_plan_kernel<SEG>, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, rp, nrows, s.cap, s.counter, s.seg_base, s.list);
    }
    return ORX_OK;
}
