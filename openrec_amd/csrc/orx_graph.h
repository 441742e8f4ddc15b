// Declarations shared by the graph propagation's translation units (kernels_graph.hip, api_csr.hip, api_lightgcn.hip).
#pragma once
#include "orx_internal.h"
#include "orx_seg_plan.h"

constexpr int GS_SEG = 512;        // entries per segment of a long row (orx_graph_segment_len)
int orx_launch_graph_spmm(orx_ctx* ctx, const float* X, int64_t M, int D, float* out, float* acc, float acc_alpha, const int64_t* rp,
                          const int32_t* cols, const float* rs, const float* cs, int64_t nrows, bool vec_ok, const SegScratch& s);
int orx_launch_graph_scale(orx_ctx* ctx, const float* in, float* out, int64_t n, float alpha);
int orx_launch_apply_dense(orx_ctx* ctx, int kind, float* w, float* s0, float* s1, const float* g, int64_t n, float lr, float eps, float b1, float b2);
int orx_graph_l2_nwaves(int64_t n);
int orx_launch_graph_l2_rows(orx_ctx* ctx, const float* W, int64_t rows, int D, const int32_t* ids, int64_t n, float coef, float* grads, float* partial);
int orx_launch_graph_concat_ids(orx_ctx* ctx, const int32_t* a, const int32_t* b, int64_t n, int32_t* out);
int orx_table_apply_dense_at(orx_ctx* c, orx_opt* opt, orx_table* t, const float* grad);
