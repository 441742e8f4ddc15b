// C-ABI entry point of WARP negative sampling: orx_sampler_pairwise_warp (kernels_warp.hip has the kernel and its design,
// include/openrec_hip.h the contract).
#include <cmath>
#include <cstring>

#include "orx_internal.h"

extern "C" int orx_sampler_pairwise_warp(orx_sampler* s, int model, orx_table* user, orx_table* item, orx_table* bias,
                                         uint64_t seed, int64_t first, int64_t n, int32_t max_trials, float margin,
                                         const float* trial_weight,
                                         int32_t* uid_dev, int32_t* pid_dev, int32_t* nid_dev, float* weight_dev,
                                         int32_t* trials_dev, float* pos_score_dev, float* cand_score_dev) {
    static const char* fn = "orx_sampler_pairwise_warp";
    ORX_ARG(s && user && item && first >= 0 && n >= 0 && (n == 0 || (uid_dev && pid_dev && nid_dev)), "%s: bad argument", fn);
    ORX_ARG(n == 0 || weight_dev, "%s: weight_dev is NULL", fn);
    ORX_ARG(trial_weight, "%s: trial_weight is NULL", fn);
    ORX_ARG(max_trials >= 1 && max_trials <= 256, "%s: max_trials must be in [1, 256], got %d", fn, max_trials);
    ORX_ARG(!std::isnan(margin), "%s: the margin is NaN", fn);
    ORX_ARG(model == ORX_BPR || model == ORX_UCML, "%s: the model must be ORX_BPR or ORX_UCML, got %d", fn, model);
    ORX_ARG(user->ctx == s->ctx && item->ctx == s->ctx && (!bias || bias->ctx == s->ctx),
            "%s: the tables live on another context than the sampler", fn);
    ORX_ARG(user->rows == s->total_users, "%s: the user table has %lld rows, the sampler %lld users", fn, (long long)user->rows,
            (long long)s->total_users);
    ORX_ARG(item->rows == s->total_items, "%s: the item table has %lld rows, the sampler %lld items", fn, (long long)item->rows,
            (long long)s->total_items);
    ORX_ARG(user->dim == item->dim, "%s: user dim %d, item dim %d", fn, user->dim, item->dim);
    ORX_ARG(!bias || (bias->rows == s->total_items && bias->dim == 1), "%s: the bias must be [items, 1]", fn);
    if (n == 0) return ORX_OK;
    // the kernel gathers rows the host does not know (they are drawn on the device): the WHOLE of a lazily-applied table is finished
    CHECK(orx_table_sync(user));
    CHECK(orx_table_sync(item));
    CHECK(orx_table_sync(bias));
    ORX_HIP(hipSetDevice(s->ctx->device));
    // the weight table: uploaded only when its floats (as bits) differ from the copy on the device.  A call enqueued earlier may
    // still read the old copy, so the stream is waited for first -- a loop that passes the same table never comes here
    if (!s->d_warpw) ORX_HIP(hipMalloc((void**)&s->d_warpw, sizeof(s->h_warpw)));
    if (s->warpw_n < max_trials || std::memcmp(s->h_warpw, trial_weight, sizeof(float) * max_trials) != 0) {
        ORX_HIP(hipStreamSynchronize(s->ctx->stream));
        s->warpw_n = 0;
        ORX_HIP(hipMemcpy(s->d_warpw, trial_weight, sizeof(float) * max_trials, hipMemcpyHostToDevice));
        std::memcpy(s->h_warpw, trial_weight, sizeof(float) * max_trials);
        s->warpw_n = max_trials;
    }
    WarpNegArgs a;
    a.s.rec_user = s->rec_user; a.s.rec_item = s->rec_item; a.s.R = s->R; a.s.ptr = s->ptr; a.s.items = s->items;
    a.s.total_items = s->total_items; a.s.total_users = s->total_users; a.s.seed = seed; a.s.first = first; a.s.n = n; a.s.h = s->h;
    a.s.uid = uid_dev; a.s.pid = pid_dev; a.s.nid = nid_dev;
    a.s.prop = s->prop_on ? s->d_prop : nullptr;
    a.U = user->w; a.V = item->w; a.b = bias ? bias->w : nullptr;
    a.model = model; a.D = user->dim; a.T = max_trials; a.margin = margin; a.tw = s->d_warpw;
    a.weight = weight_dev; a.trials = trials_dev; a.pos_score = pos_score_dev; a.cand_score = cand_score_dev;
    return orx_launch_warpneg(s->ctx, a);
}
