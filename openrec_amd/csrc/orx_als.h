// What the ALS translation units share (kernels_als.hip, kernels_als_cg.hip, api_csr.hip): the segment length, the arguments of the CG
// half-step and of the ALS objective, the launchers.
#pragma once
#include "orx_internal.h"
#include "orx_seg_plan.h"

constexpr int ALS_SEG = 1024;      // L: entries per segment of a long row, Cholesky and CG alike (orx_als_segment_len)

struct CgArgs {
    const float* F; int64_t M; int D;
    const float* Gq;                               // [Dp][Dp + 4] the full square of G, zero beyond D
    float* X;                                      // row row0 of the solved table
    const int64_t* rp; const int32_t* cols; const float* conf;      // as AlsArgs
    int64_t nrows;
    float a, b, reg;
    int cg_steps;
    // long rows
    const int* long_idx;                           // [nrows] state slot of a long row, -1: none (NULL: no plan)
    const int2* rowlist;                           // [cap_rows] (row, first scratch slot), row < 0: unused
    const int2* list;                              // [cap_slots] (state slot, segment), state slot < 0: unused
    const unsigned long long* counter;             // rows << 32 | slots handed out
    int cap_rows, cap_slots;
    float* slots;                                  // [cap_slots][2 Dp]: the segment's partial of sum w (f . v) f, then of y
    double* sx; double* sr; float* sp; double* srs;      // [cap_rows][Dp] x 3, [cap_rows]
    int* err;
};

struct ObjArgs {
    const float* U; const float* V; int64_t NU, NI; int D;
    const int64_t* rp; const int32_t* cols; const float* conf;
    int64_t nnz;
    float a, b, reg;
    double* part; int64_t nw;                      // [nw] one partial per wavefront of the pass
    const float* gramU; int nbU; const float* gramV; int nbV; int Dp16;      // slab partials of the two grams
    double* gpart; int ngw;                        // [ngw][2] the gram pass: <G_U, G_V> and the traces per workgroup
    double* out;
    int* err;
};

int orx_als_cg_breaks(int D, int32_t* out, int cap);
int64_t orx_als_cg_slot_floats(int D);
int64_t orx_als_cg_state_bytes(int D);
int64_t orx_als_cg_square_floats(int D);
int orx_launch_als_cg(orx_ctx* ctx, CgArgs p, const float* Gm, float* Gq, unsigned long long* counter, int* long_idx, int2* rowlist, int2* list);
int64_t orx_als_obj_waves(int64_t nnz);
int orx_als_obj_gram_groups(int D);
int orx_launch_als_objective(orx_ctx* ctx, ObjArgs p);
// kernels_als.hip: the slab partials of G = F^T F into gram_part [orx_als_gram_blocks(M)][Dp16 * Dp16] and, unless Gm is NULL, their
// sum in slab order into Gm [Dp16][Dp16] (tiles on and below the diagonal)
int orx_als_gram_blocks(int64_t M);
int orx_launch_als_gram(orx_ctx* ctx, const float* F, int64_t M, int D, float* gram_part, float* Gm);
// the Cholesky half-step after the gram: segment plan + partials (s.cap > 0), solve.  s.slots: [s.cap][orx_als_slot_floats(D)]
int64_t orx_als_slot_floats(int D);
int orx_launch_als(orx_ctx* ctx, const float* F, int64_t M, int D, float* X, const int64_t* rp, const int32_t* cols, const float* conf,
                   int64_t nrows, float a, float b, float reg, const float* Gm, const SegScratch& s);
