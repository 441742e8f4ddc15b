// C-ABI entry points of the one-positive-against-N-negatives objective: orx_multineg_step, orx_multineg_loss and
// orx_sampler_pairwise_multi (include/openrec_hip.h has the semantics, kernels_multineg.hip the kernels).
//
// Per step, all on the context's stream: [lazy Adam: the rows the step reads are replayed to the optimizer's step -- the user
// table with uid, the item table and the bias with pid and with nid, which together are the concatenated list], ONE gradient
// launch that writes per-occurrence gradient rows and the concatenated item id list, [Adam: the counter advances], then
// orx_apply_rows of the user table and of the item table with the bias.  The gradient launch ends before the applies begin, so
// every gradient is taken on the pre-step tables.  The loss partials of up to MN_CHUNK steps are summed by one loss_reduce launch
// (a fixed order, no atomics -- orx_launch_loss_accumulate adds its blocks' sums with fp64 atomics once there are more than 2048
// partials, which would cost loss_out its bit-repeatability) into device doubles that are read once at the end of the call.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "orx_internal.h"

namespace {

constexpr int64_t MN_CHUNK = 32;              // steps whose loss partials are summed by one launch

struct Carve {                                // consecutive 256-byte aligned pieces of one device buffer
    size_t off = 0;
    size_t take(size_t bytes) { const size_t at = off; off += (bytes + 255) & ~(size_t)255; return at; }
};

// what the step and the forward share
int check_model(const char* fn, orx_ctx* c, int kind, orx_table* U, orx_table* V, orx_table* b, int32_t N) {
    ORX_ARG(c && U && V, "%s: NULL context/table", fn);
    ORX_ARG(kind == ORX_MN_SOFTMAX || kind == ORX_MN_LOGSIG, "%s: unknown loss kind %d (ORX_MN_SOFTMAX, ORX_MN_LOGSIG)", fn, kind);
    ORX_ARG(N >= 1 && N <= 64, "%s: N must be in [1, 64], got %d", fn, N);
    ORX_ARG(U->ctx == c && V->ctx == c && (!b || b->ctx == c), "%s: the tables belong to a different context", fn);
    ORX_ARG(U->dim == V->dim, "%s: user dim %d != item dim %d (dot scores only)", fn, U->dim, V->dim);
    ORX_ARG(!b || (b->dim == 1 && b->rows == V->rows), "%s: item_bias must be [%lld, 1]", fn, (long long)V->rows);
    return ORX_OK;
}

// the inputs of K steps on the device: arrays that are there already as they are (stride ds = id_stride), host arrays packed at
// stride B into the context's staging buffers (ids: d_ids, weights and offsets: d_lab)
struct Inputs { const int32_t* du; const int32_t* dp; const int32_t* dn; const float* dw; const float* doff; int64_t ds; };

int stage_inputs(orx_ctx* c, const int32_t* uid, const int32_t* pid, const int32_t* nid, const float* weight, const float* off,
                 int64_t K, int64_t B, int64_t N, int64_t id_stride, int flags, Inputs* in) {
    if (flags & ORX_IDS_DEVICE) { *in = Inputs{uid, pid, nid, weight, off, id_stride}; return ORX_OK; }
    const int64_t n = K * B;
    ENSURE(c->d_ids, c->d_ids_cap, (size_t)n * (2 + N) * sizeof(int32_t));
    if (weight || off) ENSURE(c->d_lab, c->d_lab_cap, (size_t)n * (1 + N) * sizeof(float));
    for (int64_t s = 0; s < K; ++s) {
        CHECK(stage_ids(c, uid + s * id_stride, B, s * B));
        CHECK(stage_ids(c, pid + s * id_stride, B, n + s * B));
        CHECK(stage_ids(c, nid + s * id_stride * N, B * N, 2 * n + s * B * N));
        if (weight) ORX_HIP(hipMemcpyAsync(c->d_lab + s * B, weight + s * id_stride, (size_t)B * sizeof(float), hipMemcpyHostToDevice, c->stream));
        if (off) ORX_HIP(hipMemcpyAsync(c->d_lab + n + s * B * N, off + s * id_stride * N, (size_t)B * N * sizeof(float), hipMemcpyHostToDevice, c->stream));
    }
    *in = Inputs{c->d_ids, c->d_ids + n, c->d_ids + 2 * n, weight ? c->d_lab : nullptr, off ? c->d_lab + n : nullptr, B};
    return ORX_OK;
}

}  // namespace

extern "C" int orx_multineg_step(orx_ctx* c, int kind, orx_opt* opt, orx_table* U, orx_table* V, orx_table* b,
                                 const int32_t* uid, const int32_t* pid, const int32_t* nid, const float* weight, const float* neg_offset,
                                 int64_t K, int64_t B, int32_t N, int64_t id_stride, float l2_reg, int flags,
                                 float* loss_out, float* l2_out) {
    static const char* fn = "orx_multineg_step";
    ORX_ARG(opt, "%s: NULL optimizer", fn);
    CHECK(check_model(fn, c, kind, U, V, b, N));
    ORX_ARG(opt->ctx == c, "%s: the optimizer belongs to a different context", fn);
    ORX_ARG(!(flags & ORX_HOGWILD), "%s: ORX_HOGWILD is a speed-comparison mode of the plain pairwise step only", fn);
    ORX_ARG(!(flags & ORX_CENSOR), "%s: ORX_CENSOR belongs to UCML; this step scores by dot products only (UCML / L2 scoring is not offered)", fn);
    ORX_ARG(std::isfinite(l2_reg) && l2_reg >= 0.f, "%s: l2_reg must be finite and >= 0 (got %g)", fn, (double)l2_reg);
    ORX_ARG(!(flags & ORX_NO_L2) || l2_reg == 0.f, "%s: ORX_NO_L2 together with l2_reg = %g (drop the flag, or pass l2_reg = 0)", fn, (double)l2_reg);
    ORX_ARG(K >= 0 && B >= 0 && id_stride >= 0, "%s: negative K, B or id_stride", fn);
    // what orx_apply_rows would refuse for this optimizer and these tables, with its message, before anything is launched
    ORX_ARG(opt->kind == ORX_SGD || opt->kind == ORX_ADAGRAD || opt->kind == ORX_MOMENTUM || (opt->kind == ORX_ADAM && (!b || orx_adam_rows_lazy(opt, V))),
            "orx_apply_rows: the whole-table-sweep form of Adam (ORX_ADAM_DENSE) takes no bias column");
    if (K == 0 || B == 0) return ORX_OK;
    ORX_ARG(uid && pid && nid, "%s: NULL id pointer", fn);
    ORX_ARG(K == 1 || id_stride >= B, "%s: id_stride %lld below B = %lld", fn, (long long)id_stride, (long long)B);
    ORX_ARG((B * (1 + (int64_t)N)) <= 0x7fffffffLL, "%s: B * (1 + N) must fit 31 bits", fn);
    const bool adam = opt->kind == ORX_ADAM;
    ORX_ARG(!adam || opt->t + K < 0x7fffffff, "%s: step counter overflow", fn);
    ORX_HIP(hipSetDevice(c->device));

    Inputs in;
    CHECK(stage_inputs(c, uid, pid, nid, weight, neg_offset, K, B, N, id_stride, flags, &in));
    const int D = U->dim, gs = (D + 1 + 3) & ~3;
    const int64_t nI = B * (1 + (int64_t)N);
    const int nw = orx_multineg_nwaves(c, D, B);
    const int64_t chunk = std::min<int64_t>(K, MN_CHUNK);
    const bool want = loss_out != nullptr || l2_out != nullptr;
    ENSURE(c->d_partial, c->d_partial_cap, (size_t)chunk * nw * 2 * sizeof(float));
    if (want) ENSURE(c->d_loss, c->d_loss_cap, (size_t)K * 2 * sizeof(double));
    // scratch, one buffer reused by every step: the concatenated item ids, the gradient rows
    Carve cv;
    const size_t o_list = cv.take((size_t)nI * sizeof(int32_t));
    const size_t o_gu = cv.take((size_t)B * gs * sizeof(float));
    const size_t o_gi = cv.take((size_t)nI * gs * sizeof(float));
    ENSURE(c->d_tmp, c->d_tmp_cap, cv.off);
    char* base = reinterpret_cast<char*>(c->d_tmp);
    MultiNegArgs a;
    memset(&a, 0, sizeof(a));
    a.U = U->w; a.V = V->w; a.b = b ? b->w : nullptr;
    a.list = reinterpret_cast<int32_t*>(base + o_list);
    a.gu = reinterpret_cast<float*>(base + o_gu); a.gi = reinterpret_cast<float*>(base + o_gi);
    a.B = B; a.NU = U->rows; a.NI = V->rows; a.N = N; a.D = D; a.gs = gs;
    a.invB = 1.0f / (float)B; a.l2w = l2_reg; a.err = c->d_err;
    orx_table* tabs[3] = {U, V, b};
    const int ntabs = b ? 3 : 2;

    for (int64_t s0 = 0; s0 < K; s0 += chunk) {
        const int64_t kc = std::min<int64_t>(chunk, K - s0);
        for (int64_t i = 0; i < kc; ++i) {
            const int64_t s = s0 + i;
            a.uid = in.du + s * in.ds; a.pid = in.dp + s * in.ds; a.nid = in.dn + s * in.ds * N;
            a.wt = in.dw ? in.dw + s * in.ds : nullptr;
            a.off = in.doff ? in.doff + s * in.ds * N : nullptr;
            a.partial = c->d_partial + (size_t)i * nw * 2;
            // a lazily-applied table: exactly the rows this step reads (no-ops for a table that is current)
            CHECK(orx_table_touch(U, a.uid, B));
            CHECK(orx_table_touch(V, a.pid, B)); CHECK(orx_table_touch(V, a.nid, B * N));
            if (b) { CHECK(orx_table_touch(b, a.pid, B)); CHECK(orx_table_touch(b, a.nid, B * N)); }
            CHECK(orx_launch_multineg(c, kind, true, a));
            if (adam) CHECK(orx_opt_advance(opt, tabs, ntabs));        // once per step: after the step's reads, before its applies
            CHECK(orx_apply_rows(c, opt, U, nullptr, a.uid, B, a.gu, gs));
            CHECK(orx_apply_rows(c, opt, V, b, a.list, nI, a.gi, gs));
        }
        if (want) {
            ReduceArgs r;
            r.partial = c->d_partial; r.out = c->d_loss + 2 * s0; r.nwaves = nw;
            CHECK(orx_launch_loss_reduce(c, r, kc));
        }
    }
    CHECK(fetch_losses(c, K, loss_out, l2_out));
    if (!(flags & ORX_IDS_DEVICE)) return orx_check_index_error(c);
    return ORX_OK;
}

extern "C" int orx_multineg_loss(orx_ctx* c, int kind, orx_table* U, orx_table* V, orx_table* b,
                                 const int32_t* uid, const int32_t* pid, const int32_t* nid, const float* weight, const float* neg_offset,
                                 int64_t B, int32_t N, int flags, float* loss_out, float* l2_out) {
    static const char* fn = "orx_multineg_loss";
    CHECK(check_model(fn, c, kind, U, V, b, N));
    ORX_ARG((flags & ~ORX_IDS_DEVICE) == 0, "%s: flags other than ORX_IDS_DEVICE", fn);
    ORX_ARG(B >= 0, "%s: negative B", fn);
    if (B == 0) {
        if (loss_out) *loss_out = 0.f;
        if (l2_out) *l2_out = 0.f;
        return ORX_OK;
    }
    ORX_ARG(uid && pid && nid, "%s: NULL id pointer", fn);
    ORX_HIP(hipSetDevice(c->device));
    Inputs in;
    CHECK(stage_inputs(c, uid, pid, nid, weight, neg_offset, 1, B, N, B, flags, &in));
    const int D = U->dim;
    const int nw = orx_multineg_nwaves(c, D, B);
    ENSURE(c->d_partial, c->d_partial_cap, (size_t)nw * 2 * sizeof(float));
    ENSURE(c->d_loss, c->d_loss_cap, 2 * sizeof(double));
    CHECK(orx_table_touch(U, in.du, B));
    CHECK(orx_table_touch(V, in.dp, B)); CHECK(orx_table_touch(V, in.dn, B * N));
    if (b) { CHECK(orx_table_touch(b, in.dp, B)); CHECK(orx_table_touch(b, in.dn, B * N)); }
    MultiNegArgs a;
    memset(&a, 0, sizeof(a));
    a.U = U->w; a.V = V->w; a.b = b ? b->w : nullptr;
    a.uid = in.du; a.pid = in.dp; a.nid = in.dn; a.wt = in.dw; a.off = in.doff;
    a.B = B; a.NU = U->rows; a.NI = V->rows; a.N = N; a.D = D; a.gs = (D + 1 + 3) & ~3;
    a.invB = 1.0f / (float)B; a.l2w = 0.f; a.partial = c->d_partial; a.err = c->d_err;
    CHECK(orx_launch_multineg(c, kind, false, a));
    ReduceArgs r;
    r.partial = c->d_partial; r.out = c->d_loss; r.nwaves = nw;
    CHECK(orx_launch_loss_reduce(c, r, 1));
    float dummy;
    CHECK(fetch_losses(c, 1, loss_out ? loss_out : &dummy, l2_out));
    return orx_check_index_error(c);
}

extern "C" int orx_sampler_pairwise_multi(orx_sampler* s, uint64_t seed, int64_t first, int64_t n, int32_t n_neg,
                                          int32_t* uid_dev, int32_t* pid_dev, int32_t* nid_dev) {
    static const char* fn = "orx_sampler_pairwise_multi";
    ORX_ARG(s && first >= 0 && n >= 0 && (n == 0 || (uid_dev && pid_dev && nid_dev)), "%s: bad argument", fn);
    ORX_ARG(n_neg >= 1 && n_neg <= 64, "%s: n_neg must be in [1, 64], got %d", fn, n_neg);
    if (n == 0) return ORX_OK;
    ORX_HIP(hipSetDevice(s->ctx->device));
    SamplerArgs a;
    a.rec_user = s->rec_user; a.rec_item = s->rec_item; a.R = s->R; a.ptr = s->ptr; a.items = s->items;
    a.total_items = s->total_items; a.total_users = s->total_users; a.seed = seed; a.first = first; a.n = n; a.h = s->h;
    a.uid = uid_dev; a.pid = pid_dev; a.nid = nid_dev;
    a.prop = s->prop_on ? s->d_prop : nullptr;
    return orx_launch_sample_multi(s->ctx, a, n_neg);
}
