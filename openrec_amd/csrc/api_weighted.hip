// C-ABI entry points of the weighted objective (include/openrec_hip.h has the semantics): the pairwise step with per-triplet
// weights and an l2 coefficient, its forward, and the pointwise steps with the coefficient.  (The sampler's per-record weights,
// which deliver the weights of a pairwise draw, are in api_sampler.hip.)
//
// Nothing is computed here.  The entry points check what only they can refuse and hand over to the bodies of the plain steps
// (orx_pairwise_step_impl and its kin: api.hip, api_subset.hip, api_more.hip), which carry the two knobs as arguments: the weight
// pointer reaches the fused kernels as PairArgs::wt / SubsetArgs::wt, where a non-NULL pointer selects their compile-time weighted
// variants -- the plain entry points launch the kernels they always launched --, and l2_reg is the l2w the kernels always had.
#include <cmath>

#include "orx_internal.h"

namespace {

// what the three step entry points refuse on top of the plain steps
int check_objective(const char* fn, float l2_reg, int flags) {
    ORX_ARG(!(flags & ORX_HOGWILD), "%s: ORX_HOGWILD is a speed-comparison mode of the plain step only (no weights, no l2 coefficient)", fn);
    ORX_ARG(std::isfinite(l2_reg) && l2_reg >= 0.f, "%s: l2_reg must be finite and >= 0 (got %g)", fn, (double)l2_reg);
    ORX_ARG(!(flags & ORX_NO_L2) || l2_reg == 0.f, "%s: ORX_NO_L2 together with l2_reg = %g (drop the flag, or pass l2_reg = 0)", fn, (double)l2_reg);
    return ORX_OK;
}

}  // namespace

extern "C" int orx_pairwise_step_weighted(orx_ctx* c, int model, orx_opt* opt, orx_table* U, orx_table* V, orx_table* b,
                                          const int32_t* uid, const int32_t* pid, const int32_t* nid, const float* weight,
                                          int64_t K, int64_t B, int64_t id_stride, float margin, float l2_reg, int flags,
                                          int train_mask, float* loss_out, float* l2_out) {
    CHECK(check_objective("orx_pairwise_step_weighted", l2_reg, flags));
    if (train_mask == 0) return orx_pairwise_step_impl(c, model, opt, U, V, b, uid, pid, nid, weight, K, B, id_stride, margin, l2_reg, flags, loss_out, l2_out);
    return orx_pairwise_subset_impl(c, model, opt, U, V, b, uid, pid, nid, weight, K, B, id_stride, margin, l2_reg, flags, train_mask, loss_out, l2_out);
}

extern "C" int orx_pairwise_loss_weighted(orx_ctx* c, int model, orx_table* U, orx_table* V, orx_table* b,
                                          const int32_t* uid, const int32_t* pid, const int32_t* nid, const float* weight,
                                          int64_t B, float margin, int flags, float* loss_out, float* l2_out) {
    return orx_pairwise_loss_impl(c, model, U, V, b, uid, pid, nid, weight, B, margin, flags, loss_out, l2_out);
}

extern "C" int orx_pointwise_step_l2reg(orx_ctx* c, int model, orx_opt* opt, orx_table* U, orx_table* V, orx_table* b, orx_table* w,
                                        const int32_t* uid, const int32_t* iid, const float* label,
                                        int64_t K, int64_t B, int64_t id_stride, float a_w, float b_w, float l2_reg, int flags,
                                        int train_mask, float* loss_out, float* l2_out) {
    CHECK(check_objective("orx_pointwise_step_l2reg", l2_reg, flags));
    if (train_mask == 0) return orx_pointwise_step_impl(c, model, opt, U, V, b, w, uid, iid, label, K, B, id_stride, a_w, b_w, l2_reg, flags, loss_out, l2_out);
    return orx_pointwise_subset_impl(c, model, opt, U, V, b, w, uid, iid, label, K, B, id_stride, a_w, b_w, l2_reg, flags, train_mask, loss_out, l2_out);
}
