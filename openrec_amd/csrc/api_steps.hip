// The host driver the train steps on per-occurrence gradient rows share (orx_internal.h has the contracts): staging of K steps'
// lists, the argument checks of a dot-score family, the touch of the lazy rows, the chunked step loop with its loss sums, the
// forward-only tail, the sort that is kept aside and the apply of a sorted list.  Host code only; DESIGN 4 says what a new step
// family supplies.
#include <algorithm>
#include <cmath>

#include "orx_internal.h"

// one list: K pieces of B * width elements, id_stride * width apart on the host, packed at dst
static int copy_list(orx_ctx* c, const StepList& l, void* dst, int64_t K, int64_t B, int64_t id_stride) {
    const size_t piece = (size_t)B * l.width * 4;
    if (id_stride == B || K == 1) {
        ORX_HIP(hipMemcpyAsync(dst, l.p, (size_t)K * piece, hipMemcpyHostToDevice, c->stream));
        return ORX_OK;
    }
    for (int64_t s = 0; s < K; ++s)
        ORX_HIP(hipMemcpyAsync((char*)dst + s * piece, (const char*)l.p + (size_t)s * id_stride * l.width * 4, piece, hipMemcpyHostToDevice, c->stream));
    return ORX_OK;
}

int orx_stage_steps(orx_ctx* c, int64_t K, int64_t B, int64_t id_stride, int flags, std::initializer_list<StepList> ids,
                    std::initializer_list<StepList> floats, StepInputs* in) {
    const bool dev = (flags & ORX_IDS_DEVICE) != 0;
    *in = StepInputs{{nullptr, nullptr, nullptr}, {nullptr, nullptr}, dev ? id_stride : B};
    const int64_t n = K * B;
    size_t n_ids = 0, n_flt = 0;              // both buffers are sized before the first copy into them
    for (const StepList& l : ids) if (l.p) n_ids += (size_t)n * l.width;
    for (const StepList& l : floats) if (l.p) n_flt += (size_t)n * l.width;
    if (!dev && n_ids) ENSURE(c->d_ids, c->d_ids_cap, n_ids * sizeof(int32_t));
    if (!dev && n_flt) ENSURE(c->d_lab, c->d_lab_cap, n_flt * sizeof(float));
    size_t at = 0; int k = 0;
    for (const StepList& l : ids) {
        if (l.p && !dev) { CHECK(copy_list(c, l, c->d_ids + at, K, B, id_stride)); in->id[k] = c->d_ids + at; at += (size_t)n * l.width; }
        else in->id[k] = static_cast<const int32_t*>(l.p);
        ++k;
    }
    at = 0; k = 0;
    for (const StepList& l : floats) {
        if (l.p && !dev) { CHECK(copy_list(c, l, c->d_lab + at, K, B, id_stride)); in->f[k] = c->d_lab + at; at += (size_t)n * l.width; }
        else in->f[k] = static_cast<const float*>(l.p);
        ++k;
    }
    return ORX_OK;
}

int orx_run_steps(orx_ctx* c, int64_t K, int np, int flags, float* loss_out, float* l2_out,
                  const std::function<int(int64_t, int64_t)>& chunk, const std::function<int(int64_t, int64_t, float*)>& step) {
    const int64_t nc = std::min<int64_t>(K, ORX_STEP_CHUNK);
    const bool want = loss_out != nullptr || l2_out != nullptr;
    ENSURE(c->d_partial, c->d_partial_cap, (size_t)nc * np * 2 * sizeof(float));
    if (want) ENSURE(c->d_loss, c->d_loss_cap, (size_t)K * 2 * sizeof(double));
    for (int64_t s0 = 0; s0 < K; s0 += nc) {
        const int64_t kc = std::min<int64_t>(nc, K - s0);
        if (chunk) CHECK(chunk(s0, kc));
        for (int64_t i = 0; i < kc; ++i) CHECK(step(s0 + i, i, c->d_partial + (size_t)i * np * 2));
        if (want) {         // a fixed order, no atomics: the sums are bit-repeatable; nothing reads d_loss but the fetch below
            ReduceArgs r;
            r.partial = c->d_partial; r.out = c->d_loss + 2 * s0; r.nwaves = np;
            CHECK(orx_launch_loss_reduce(c, r, kc));
        }
    }
    CHECK(fetch_losses(c, K, loss_out, l2_out));
    if (!(flags & ORX_IDS_DEVICE)) return orx_check_index_error(c);
    return ORX_OK;
}

int orx_run_forward(orx_ctx* c, int np, float* loss_out, float* l2_out, const std::function<int(float*)>& forward) {
    ENSURE(c->d_partial, c->d_partial_cap, (size_t)np * 2 * sizeof(float));
    ENSURE(c->d_loss, c->d_loss_cap, 2 * sizeof(double));
    CHECK(forward(c->d_partial));
    ReduceArgs r;
    r.partial = c->d_partial; r.out = c->d_loss; r.nwaves = np;
    CHECK(orx_launch_loss_reduce(c, r, 1));
    float dummy;                              // (the call synchronises whatever the caller asks for)
    CHECK(fetch_losses(c, 1, loss_out ? loss_out : &dummy, l2_out));
    return orx_check_index_error(c);
}

int orx_check_dot_model(const char* fn, orx_ctx* c, orx_table* U, orx_table* V, orx_table* b, int extra_dim, int flags, int allowed) {
    ORX_ARG(c && U && V, "%s: NULL context/table", fn);
    ORX_ARG(U->ctx == c && V->ctx == c && (!b || b->ctx == c), "%s: the tables belong to a different context", fn);
    ORX_ARG(U->dim == V->dim + extra_dim, "%s: user dim %d != item dim %d (dot scores only)", fn, U->dim, V->dim + extra_dim);
    ORX_ARG(!b || (b->dim == 1 && b->rows == V->rows), "%s: item_bias must be [%lld, 1]", fn, (long long)V->rows);
    ORX_ARG((flags & ~allowed) == 0, "%s: unknown flags", fn);
    ORX_ARG(!(flags & ORX_HOGWILD), "%s: ORX_HOGWILD is a speed-comparison mode of the plain pairwise step only", fn);
    ORX_ARG(!(flags & ORX_CENSOR), "%s: ORX_CENSOR belongs to UCML; this step scores by dot products only (UCML / L2 scoring is not offered)", fn);
    return ORX_OK;
}

int orx_check_apply_rows_opt(const orx_opt* opt, const orx_table* t, const orx_table* bias) {
    ORX_ARG(opt->kind == ORX_SGD || opt->kind == ORX_ADAGRAD || opt->kind == ORX_MOMENTUM || (opt->kind == ORX_ADAM && (!bias || orx_adam_rows_lazy(opt, t))),
            "orx_apply_rows: the whole-table-sweep form of Adam (ORX_ADAM_DENSE) takes no bias column");
    return ORX_OK;
}

int orx_check_dot_step(const char* fn, orx_ctx* c, orx_opt* opt, orx_table* U, orx_table* V, orx_table* b, int extra_dim,
                       int64_t K, int64_t B, int64_t id_stride, float l2_reg, int flags, int allowed) {
    ORX_ARG(opt, "%s: NULL optimizer", fn);
    CHECK(orx_check_dot_model(fn, c, U, V, b, extra_dim, flags, allowed));
    ORX_ARG(opt->ctx == c, "%s: the optimizer belongs to a different context", fn);
    ORX_ARG(std::isfinite(l2_reg) && l2_reg >= 0.f, "%s: l2_reg must be finite and >= 0 (got %g)", fn, (double)l2_reg);
    ORX_ARG(!(flags & ORX_NO_L2) || l2_reg == 0.f, "%s: ORX_NO_L2 together with l2_reg = %g (drop the flag, or pass l2_reg = 0)", fn, (double)l2_reg);
    ORX_ARG(K >= 0 && B >= 0 && id_stride >= 0, "%s: negative K, B or id_stride", fn);
    // what the step's applies would refuse for this optimizer and these tables, before anything is launched
    CHECK(orx_check_apply_rows_opt(opt, V, b));
    const bool empty = K == 0 || B == 0;      // such a call returns before it looks at its lists: nothing below refuses it
    ORX_ARG(empty || K == 1 || id_stride >= B, "%s: id_stride %lld below B = %lld", fn, (long long)id_stride, (long long)B);
    ORX_ARG(empty || opt->kind != ORX_ADAM || opt->t + K < 0x7fffffff, "%s: step counter overflow", fn);
    return ORX_OK;
}

int orx_touch_step(orx_table* U, orx_table* V, orx_table* b, const int32_t* uid, int64_t nu, const int32_t* i0, int64_t n0,
                   const int32_t* i1, int64_t n1) {
    CHECK(orx_table_touch(U, uid, nu));
    CHECK(orx_table_touch(V, i0, n0));
    if (i1) CHECK(orx_table_touch(V, i1, n1));
    CHECK(orx_table_touch(b, i0, n0));        // (no bias table: a no-op)
    if (i1) CHECK(orx_table_touch(b, i1, n1));
    return ORX_OK;
}

int orx_rows_sort_keep(orx_ctx* c, const int32_t* ids, int64_t K, int64_t n, int64_t id_stride, int64_t rows, uint2* keep) {
    const uint2* sorted = nullptr;
    CHECK(orx_rows_sort(c, ids, K, n, id_stride, rows, &sorted));
    ORX_HIP(hipMemcpyAsync(keep, sorted, (size_t)K * n * sizeof(uint2), hipMemcpyDeviceToDevice, c->stream));
    return ORX_OK;
}

int orx_apply_rows_sorted(orx_ctx* c, orx_opt* opt, orx_table* t, const uint2* sorted, int64_t n, const float* grads, int64_t g_stride) {
    if (orx_adam_rows_lazy(opt, t)) return orx_adam_rows_sorted(c, opt, t, sorted, n, grads, g_stride, true);
    CHECK(orx_table_sync(t));                 // (a no-op on a table that is current)
    if (opt->kind == ORX_ADAM) return orx_adam_dense_sorted(c, opt, t, sorted, n, grads, g_stride);
    return orx_csr_apply(c, opt, t, sorted, n, grads, g_stride);
}
