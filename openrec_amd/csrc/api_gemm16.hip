// Diagnostic entry points of the fp16 MLP products (kernels_gemm16.hip): each product, the grouped launch, the head's kernels and the cast
// alone on caller-owned device buffers, and a query of what the launchers choose for a shape.  tests/test_gpu_gemm16.py compares every one
// with an exact reference; the DLRM step (dlrm.hip) calls the same launchers.  Thin: argument checks, then the launcher on the context's stream.
#include "orx_internal.h"

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int orx_gemm16_plan(int32_t num_cu, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb, int32_t* nt_out, int32_t* tn_out) {
    ORX_ARG(num_cu > 0 && M > 0 && N > 0 && K > 0 && lda >= 0 && ldb >= 0 && nt_out && tn_out, "orx_gemm16_plan: bad argument");
    const Nt16Plan n = orx_gemm16_nt_plan(num_cu, M, N, lda, ldb);
    nt_out[0] = n.cfg; nt_out[1] = n.stages; nt_out[2] = n.tail; nt_out[3] = n.wave_tile; nt_out[4] = n.bm; nt_out[5] = n.bn;
    nt_out[6] = (int32_t)n.blocks; nt_out[7] = (int32_t)n.mask_words;
    const Tn16Plan t = orx_gemm16_tn_form(num_cu, M, N, K, lda, ldb);
    tn_out[0] = t.S; tn_out[1] = t.tiles; tn_out[2] = t.kchunk; tn_out[3] = t.form; tn_out[4] = t.tail;
    for (int i = 5; i < 8; ++i) tn_out[i] = 0;
    return ORX_OK;
}

extern "C" int orx_gemm16_group_query(int32_t num_cu, int32_t B, int32_t in, int32_t out, int64_t ldx, int64_t lddz, int64_t ldw, int32_t nt_cols,
                                      int32_t* plan_out) {
    ORX_ARG(num_cu > 0 && B > 0 && in > 0 && out > 0 && nt_cols >= 0 && plan_out, "orx_gemm16_group_query: bad argument");
    const Group16Plan p = orx_gemm16_group_plan(num_cu, B, in, out, ldx, lddz, ldw, nt_cols);
    plan_out[0] = p.grouped; plan_out[1] = p.tn_tail; plan_out[2] = p.nt_tail; plan_out[3] = p.S; plan_out[4] = p.tiles; plan_out[5] = p.kchunk;
    plan_out[6] = p.n_tn; plan_out[7] = p.n_nt;
    return ORX_OK;
}

extern "C" int orx_gemm16_nt(orx_ctx* c, const void* A16, int64_t lda, const void* B16, int64_t ldb, float* C, int64_t ldc, void* C16, int64_t ldc16,
                             const float* bias, int32_t M, int32_t N, int32_t K, int act, const float* actY, const void* actY16, int64_t ldy, int act_y,
                             float* colparts, int32_t* P_out, void* mask_out, const void* mask_in) {
    ORX_ARG(c && A16 && B16 && M > 0 && N > 0 && K > 0, "orx_gemm16_nt: bad argument");
    ORX_ARG(lda % 8 == 0 && ldb % 8 == 0 && aligned16(A16) && aligned16(B16), "orx_gemm16_nt: operands need 16-byte rows");
    ORX_ARG(orx_gemm16_nt_ok(lda, ldb, N, K) && K <= lda && K <= ldb, "orx_gemm16_nt: N >= 32, 8 <= K <= lda, ldb");
    ORX_ARG((C || C16) && (!C || (ldc >= N && aligned16(C))) && (!C16 || (ldc16 >= N && aligned16(C16))), "orx_gemm16_nt: outputs");
    ORX_ARG(act >= 0 && act <= 2 && act_y >= 0 && act_y <= 2 && !(actY && actY16) && ((!actY && !actY16) || ldy >= N) &&
            (!actY || aligned16(actY)) && (!actY16 || aligned16(actY16)) && (!bias || aligned16(bias)), "orx_gemm16_nt: epilogue arguments");
    ORX_ARG(!colparts || actY || actY16 || mask_in, "orx_gemm16_nt: column sums belong to the fused activation backward");
    ORX_ARG(!mask_in || (act_y == 1 && actY16 && !actY), "orx_gemm16_nt: mask_in stands for the relu backward of actY16");
    ColPart gb{colparts, 0};
    const int rc = orx_launch_gemm16_nt(c, A16, lda, B16, ldb, C, ldc, C16, ldc16, bias, M, N, K, act, actY, actY16, ldy, act_y, colparts ? &gb : nullptr,
                                        (unsigned long long*)mask_out, (const unsigned long long*)mask_in);
    if (P_out) *P_out = gb.P;
    return rc;
}

extern "C" int orx_gemm16_tn(orx_ctx* c, const void* A16, int64_t lda, const void* B16, int64_t ldb, float* C, int64_t ldc, float* slab,
                             int32_t M, int32_t N, int32_t K, float out_scale) {
    ORX_ARG(c && A16 && B16 && C && M > 0 && N > 0 && K > 0 && ldc >= N, "orx_gemm16_tn: bad argument");
    ORX_ARG(lda % 8 == 0 && ldb % 8 == 0 && aligned16(A16) && aligned16(B16), "orx_gemm16_tn: operands need 16-byte rows");
    ORX_ARG(orx_gemm16_tn_ok(lda, ldb, N) && lda >= M && ldb >= N && aligned16(C) && aligned16(slab), "orx_gemm16_tn: N % 8 == 0, lda >= M, ldb >= N");
    int S, tiles, kchunk;
    orx_gemm16_tn_plan(c, M, N, K, &S, &tiles, &kchunk);
    ORX_ARG(S == 1 || slab != nullptr, "orx_gemm16_tn: split-K needs a slab workspace");
    int rc = orx_launch_gemm16_tn(c, A16, lda, B16, ldb, C, ldc, slab, M, N, K, out_scale);
    if (rc != ORX_OK || S == 1) return rc;
    // the slices' sum, as the DLRM backward runs it: one job, one launch (the descriptor lives on the device for the launch's duration)
    SlabReduce j; j.slab = slab; j.C = C; j.ldc = ldc; j.M = M; j.N = N; j.S = S; j.ntn = (N + 127) / 128; j.tiles = tiles;
    SlabReduce* d_job = nullptr;
    ORX_HIP(hipMalloc((void**)&d_job, sizeof(SlabReduce)));
    hipError_t e = hipMemcpy(d_job, &j, sizeof(SlabReduce), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        rc = orx_launch_slab_reduce(c, d_job, 1, tiles, out_scale);
        e = hipStreamSynchronize(c->stream);
    }
    (void)hipFree(d_job);
    ORX_HIP(e);
    return rc;
}

extern "C" int orx_gemm16_group(orx_ctx* c, const void* X16, int64_t ldx, const void* dZ16, int64_t lddz, float* gW, int64_t ldgw, float* slab,
                                int32_t in, int32_t out, int32_t B, float out_scale, const void* W16, int64_t ldw, float* C, int64_t ldc,
                                void* C16, int64_t ldc16, const float* actY, const void* actY16, int64_t ldy, int act_y, float* colparts,
                                int32_t* P_out, const void* mask_in, int32_t nt_cols) {
    ORX_ARG(c && X16 && dZ16 && W16 && gW && in > 0 && out > 0 && B > 0 && ldgw >= out && nt_cols >= 0, "orx_gemm16_group: bad argument");
    const int in_nt = nt_cols > 0 ? nt_cols : in;
    ORX_ARG(ldx % 8 == 0 && lddz % 8 == 0 && ldw % 8 == 0 && aligned16(X16) && aligned16(dZ16) && aligned16(W16), "orx_gemm16_group: operands need 16-byte rows");
    ORX_ARG(in_nt >= in && orx_gemm16_nt_ok(lddz, ldw, in_nt, out) && orx_gemm16_tn_ok(ldx, lddz, out) && ldx >= in && lddz >= out && ldw >= out &&
            (int64_t)B * lddz < (1LL << 29) && (int64_t)in_nt * ldw < (1LL << 29) && (int64_t)B * ldx < (1LL << 29) && aligned16(gW) && aligned16(slab),
            "orx_gemm16_group: shapes the grouped kernel does not carry");
    ORX_ARG((C || C16) && (!C || (ldc >= in_nt && aligned16(C))) && (!C16 || (ldc16 >= in_nt && aligned16(C16))), "orx_gemm16_group: outputs");
    ORX_ARG(act_y >= 0 && act_y <= 2 && !(actY && actY16) && ((!actY && !actY16) || ldy >= in_nt) && (!actY || aligned16(actY)) && (!actY16 || aligned16(actY16)),
            "orx_gemm16_group: epilogue arguments");
    ORX_ARG(!colparts || actY || actY16 || mask_in, "orx_gemm16_group: column sums belong to the fused activation backward");
    ORX_ARG(!mask_in || (act_y == 1 && actY16 && !actY), "orx_gemm16_group: mask_in stands for the relu backward of actY16");
    const Group16Plan p = orx_gemm16_group_plan(c->num_cu, B, in, out, ldx, lddz, ldw, nt_cols);
    ORX_ARG(p.S == 1 || slab != nullptr, "orx_gemm16_group: split-K needs a slab workspace");
    ColPart gb{colparts, 0};
    int rc = orx_launch_gemm16_group(c, X16, ldx, dZ16, lddz, gW, ldgw, slab, in, out, B, out_scale, W16, ldw, C, ldc, C16, ldc16, actY, actY16, ldy, act_y,
                                     colparts ? &gb : nullptr, (const unsigned long long*)mask_in, nt_cols);
    if (P_out) *P_out = gb.P;
    if (rc != ORX_OK || p.S == 1) return rc;
    SlabReduce j; j.slab = slab; j.C = gW; j.ldc = ldgw; j.M = in; j.N = out; j.S = p.S; j.ntn = (out + 127) / 128; j.tiles = p.tiles;
    SlabReduce* d_job = nullptr;
    ORX_HIP(hipMalloc((void**)&d_job, sizeof(SlabReduce)));
    hipError_t e = hipMemcpy(d_job, &j, sizeof(SlabReduce), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        rc = orx_launch_slab_reduce(c, d_job, 1, p.tiles, out_scale);
        e = hipStreamSynchronize(c->stream);
    }
    (void)hipFree(d_job);
    ORX_HIP(e);
    return rc;
}

extern "C" int orx_head16_fwd(orx_ctx* c, const void* X16, int64_t ldx, const void* w16, const float* bias, int act, float* pred, int32_t B, int32_t K) {
    ORX_ARG(c && X16 && w16 && bias && pred && B > 0 && act >= 0 && act <= 2, "orx_head16_fwd: bad argument");
    ORX_ARG(orx_head16_ok(K, ldx) && K <= ldx && aligned16(X16) && aligned16(w16), "orx_head16_fwd: K % 8 == 0, 8 <= K <= 1024, ldx % 8 == 0, 16-byte rows");
    return orx_launch_head_fwd(c, X16, ldx, w16, bias, act, pred, B, K);
}

extern "C" int32_t orx_head16_bwd_blocks(orx_ctx* c, int32_t B) { return c && B > 0 ? orx_head_bwd_blocks(c, B) : 0; }

extern "C" int orx_head16_bwd(orx_ctx* c, const void* X16, int64_t ldx, const void* w16, const float* dy, const float* pred, int act, int act_below,
                              float* gW_parts, float* gb_parts, void* dZ16, int64_t ld16, float* dZ32, int64_t ld32, float* gb_below_parts,
                              int32_t B, int32_t K, int32_t* P_out) {
    ORX_ARG(c && X16 && w16 && dy && pred && gW_parts && gb_parts && dZ16 && gb_below_parts && B > 0 && act >= 0 && act <= 2 && act_below >= 0 && act_below <= 2,
            "orx_head16_bwd: bad argument");
    ORX_ARG(orx_head16_ok(K, ldx) && K <= ldx && aligned16(X16) && aligned16(w16) && ld16 % 8 == 0 && ld16 >= K && aligned16(dZ16) && (!dZ32 || ld32 >= K),
            "orx_head16_bwd: K % 8 == 0, 8 <= K <= 1024, leading dimensions % 8 == 0, 16-byte rows");
    ColPart gW{gW_parts, 0}, gb{gb_parts, 0}, gbb{gb_below_parts, 0};
    const int rc = orx_launch_head_bwd(c, X16, ldx, w16, dy, pred, act, act_below, &gW, &gb, dZ16, ld16, dZ32, ld32, &gbb, B, K, nullptr);
    if (P_out) *P_out = gW.P;
    return rc;
}

extern "C" int orx_cast16(orx_ctx* c, const float* src, int64_t lds, void* dst16, int64_t ld16, int32_t M, int32_t N) {
    ORX_ARG(c && src && dst16 && M > 0 && N > 0 && lds >= N && ld16 >= N, "orx_cast16: bad argument");
    return orx_launch_cast16(c, src, lds, dst16, ld16, M, N);
}
