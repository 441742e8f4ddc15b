// C-ABI entry point of dynamic negative sampling: orx_sampler_pairwise_hard (kernels_hardneg.hip has the semantics and the design).
#include "orx_internal.h"

extern "C" int orx_sampler_pairwise_hard(orx_sampler* s, int model, orx_table* user, orx_table* item, orx_table* bias,
                                         uint64_t seed, int64_t first, int64_t n, int32_t n_cand,
                                         int32_t* uid_dev, int32_t* pid_dev, int32_t* nid_dev,
                                         int32_t* cand_dev, float* cand_score_dev) {
    static const char* fn = "orx_sampler_pairwise_hard";
    ORX_ARG(s && user && item && first >= 0 && n >= 0 && (n == 0 || (uid_dev && pid_dev && nid_dev)), "%s: bad argument", fn);
    ORX_ARG(n_cand >= 1 && n_cand <= 64, "%s: n_cand must be in [1, 64], got %d", fn, n_cand);
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
    HardNegArgs a;
    a.s.rec_user = s->rec_user; a.s.rec_item = s->rec_item; a.s.R = s->R; a.s.ptr = s->ptr; a.s.items = s->items;
    a.s.total_items = s->total_items; a.s.total_users = s->total_users; a.s.seed = seed; a.s.first = first; a.s.n = n; a.s.h = s->h;
    a.s.uid = uid_dev; a.s.pid = pid_dev; a.s.nid = nid_dev;
    a.s.prop = s->prop_on ? s->d_prop : nullptr;
    a.U = user->w; a.V = item->w; a.b = bias ? bias->w : nullptr;
    a.model = model; a.D = user->dim; a.M = n_cand; a.cand = cand_dev; a.cand_score = cand_score_dev;
    return orx_launch_hardneg(s->ctx, a);
}
