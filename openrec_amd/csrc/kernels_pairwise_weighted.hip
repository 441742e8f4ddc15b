// The fused pairwise step kernels with per-triplet weights (orx_pairwise_step_weighted / orx_pairwise_loss_weighted): the WT = true
// instantiations of orx_fused_device.h, in a translation unit of their own so that they build beside kernels_pairwise.hip's.
// Every variant the plain step has is here -- BPR, UCML, bias-free; the four optimizers and lazy Adam's three replays; censor,
// staging; exact, accumulate and loss-only modes -- except hogwild, which the weighted step refuses.
#include "orx_fused_device.h"

int orx_launch_fused_weighted(orx_ctx* ctx, int model, int optkind, int mode, const PairArgs& a) {
    if (mode == MODE_HOGWILD) { orx_set_error("fused: no weighted hogwild kernels"); return ORX_ERR_ARG; }
    return launch_fused_any<true>(ctx, model, optkind, mode, a);
}
