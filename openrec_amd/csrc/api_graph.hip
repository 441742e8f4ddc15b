// C-ABI entry points of the graph propagation and the dense optimizer apply: orx_graph_spmm, orx_graph_segment_len,
// orx_table_apply_dense (kernels_graph.hip has the kernels and the design; include/openrec_hip.h the contract).
#include "orx_internal.h"
#include "orx_graph.h"

constexpr size_t GRAPH_SLOT_BUDGET = (size_t)1 << 28;    // most scratch the partial sums of long rows may take when only the device knows the CSR

extern "C" int32_t orx_graph_segment_len(void) { return orx_graph_seg_len(); }

static size_t graph_up(size_t x) { return (x + 255) & ~(size_t)255; }

extern "C" int orx_graph_spmm(orx_ctx* c, orx_table* X, orx_table* out, orx_table* acc, float acc_alpha,
                              const int64_t* row_ptr, const int32_t* cols, const float* row_scale, const float* col_scale,
                              int64_t row0, int64_t nrows, int64_t long_segments, int flags) {
    static const char* fn = "orx_graph_spmm";
    ORX_ARG(c && X && out, "%s: NULL context or table", fn);
    ORX_ARG(X != out && X != acc, "%s: X is also the output or the accumulator", fn);
    ORX_ARG(out != acc, "%s: out and acc are the same table", fn);
    ORX_ARG(X->w != out->w && (!acc || (X->w != acc->w && out->w != acc->w)), "%s: two of the tables share their memory", fn);
    ORX_ARG(X->ctx == c && out->ctx == c && (!acc || acc->ctx == c), "%s: the tables live on another context", fn);
    ORX_ARG(X->dim == out->dim && (!acc || acc->dim == out->dim), "%s: X dim %d, out dim %d, acc dim %d", fn, X->dim, out->dim, acc ? acc->dim : out->dim);
    ORX_ARG(X->dim >= 1 && X->dim <= 128, "%s: dim %d outside [1, 128]", fn, X->dim);
    ORX_ARG(!acc || acc->rows == out->rows, "%s: acc has %lld rows, out %lld", fn, (long long)(acc ? acc->rows : 0), (long long)out->rows);
    ORX_ARG((flags & ~ORX_IDS_DEVICE) == 0, "%s: unknown flags 0x%x", fn, flags);
    ORX_ARG(row0 >= 0 && nrows >= 0 && row0 <= out->rows && nrows <= out->rows - row0,
            "%s: rows [%lld, %lld) outside out's %lld rows", fn, (long long)row0, (long long)(row0 + nrows), (long long)out->rows);
    if (nrows == 0) return ORX_OK;
    ORX_ARG(row_ptr, "%s: NULL row_ptr", fn);
    const bool dev = (flags & ORX_IDS_DEVICE) != 0;
    const int D = X->dim;
    const int64_t M = X->rows, S = orx_graph_seg_len();
    const size_t slot_bytes = (size_t)D * sizeof(float);

    // how many scratch slots the segments of long rows may take
    int64_t e_first = 0, e_count = 0, cap = 0;
    if (!dev) {
        e_first = row_ptr[row0];
        ORX_ARG(e_first >= 0, "%s: row_ptr[%lld] is negative", fn, (long long)row0);
        for (int64_t i = 0; i < nrows; ++i) {
            const int64_t n = row_ptr[row0 + i + 1] - row_ptr[row0 + i];
            ORX_ARG(n >= 0, "%s: row_ptr decreases at row %lld", fn, (long long)(row0 + i));
            if (n > S) cap += (n + S - 1) / S;
        }
        e_count = row_ptr[row0 + nrows] - e_first;
        ORX_ARG(e_count == 0 || cols, "%s: NULL cols", fn);
    } else {
        ORX_ARG(cols, "%s: NULL cols", fn);
        // long_segments >= 0: the caller counted the segments of the CSR's rows of more than S entries once (an upper bound for any
        // row range; 0: no plan, no segment launch, no scratch).  A count that is too small costs nothing but time: rows that find
        // no slot walk their segments themselves.  < 0: unknown -- the columns of a row are distinct, so none is longer than M
        const int64_t budget = (int64_t)(GRAPH_SLOT_BUDGET / slot_bytes);
        if (long_segments >= 0) cap = long_segments < budget ? long_segments : budget;
        else if (M > S) {
            const int64_t per_row = (M + S - 1) / S;
            cap = nrows < budget / per_row ? nrows * per_row : budget;
        }
    }
    const int64_t budget_all = (int64_t)1 << 24;           // the plan's slot numbers are ints
    if (cap > budget_all) cap = budget_all;

    // the tables as every reader sees them: a lazily-applied Adam is finished first
    CHECK(orx_table_sync(X));
    CHECK(orx_table_sync(out));
    if (acc) CHECK(orx_table_sync(acc));
    ORX_HIP(hipSetDevice(c->device));

    // d_topk: row offsets (host CSR) | counter | slot base per row | segment list
    const size_t o_rp = 0, o_cnt = o_rp + graph_up(dev ? 0 : (size_t)(nrows + 1) * sizeof(int64_t)), o_base = o_cnt + 256,
                 o_list = o_base + graph_up(cap ? (size_t)nrows * sizeof(int) : 0), total = o_list + graph_up((size_t)cap * sizeof(int2));
    ENSURE(c->d_topk, c->d_topk_cap, total);
    if (cap) ENSURE(c->d_splitk, c->d_splitk_cap, (size_t)cap * slot_bytes);
    const int64_t* d_rp = row_ptr + row0;
    const int32_t* d_cols = cols;
    if (!dev) {
        std::vector<int64_t> rp((size_t)nrows + 1);
        for (int64_t i = 0; i <= nrows; ++i) rp[(size_t)i] = row_ptr[row0 + i] - e_first;      // entry 0 = the first staged entry
        int64_t* drp = reinterpret_cast<int64_t*>(c->d_topk + o_rp);
        ORX_HIP(hipMemcpyAsync(drp, rp.data(), rp.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        ENSURE(c->d_ids, c->d_ids_cap, (size_t)(e_count ? e_count : 1) * sizeof(int32_t));
        if (e_count) ORX_HIP(hipMemcpyAsync(c->d_ids, cols + e_first, (size_t)e_count * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        ORX_HIP(hipStreamSynchronize(c->stream));          // `rp` is a local: its copy must have left before it goes
        d_rp = drp; d_cols = c->d_ids;
    }
    const bool vec_ok = D % 4 == 0 && (uintptr_t)X->w % 16 == 0 && (uintptr_t)out->w % 16 == 0 && (!acc || (uintptr_t)acc->w % 16 == 0) &&
                        (uintptr_t)c->d_splitk % 16 == 0;
    CHECK(orx_launch_graph_spmm(c, X->w, M, D, out->w + (size_t)row0 * D, acc ? acc->w + (size_t)row0 * D : nullptr, acc_alpha, d_rp, d_cols,
                                row_scale ? row_scale + row0 : nullptr, col_scale, nrows, vec_ok, (int)cap,
                                reinterpret_cast<unsigned long long*>(c->d_topk + o_cnt), reinterpret_cast<int*>(c->d_topk + o_base),
                                reinterpret_cast<int2*>(c->d_topk + o_list), c->d_splitk));
    out->version++;
    if (acc) acc->version++;
    if (!dev) return orx_check_index_error(c);
    return ORX_OK;
}

// the rule on one table at the step the optimizer's counter stands at.  The caller has finished a lazily-applied Adam on the table
// (orx_table_sync: every row current at the step before, the table has left the lazy set) and only then advanced the counter.
int orx_table_apply_dense_at(orx_ctx* c, orx_opt* opt, orx_table* t, const float* grad) {
    OptSlots st;
    CHECK(orx_opt_slots(opt, t, &st));
    float lr = opt->lr, eps = orx_rule_eps(opt), b1 = 0.f, b2 = 0.f;
    if (opt->kind == ORX_ADAM) {
        CHECK(orx_adam_lrt(opt, opt->t));
        lr = opt->h_lrt[(size_t)opt->t]; b1 = opt->p0; b2 = opt->p1; eps = opt->p2;
    }
    CHECK(orx_launch_apply_dense(c, opt->kind, t->w, st.s0, st.s1, grad, t->rows * t->dim, lr, eps, b1, b2));
    t->version++;
    return ORX_OK;
}

extern "C" int orx_table_apply_dense(orx_ctx* c, orx_opt* opt, orx_table* t, const float* grad) {
    static const char* fn = "orx_table_apply_dense";
    ORX_ARG(c && opt && t && grad, "%s: NULL argument", fn);
    ORX_ARG(t->ctx == c && opt->ctx == c, "%s: the table or the optimizer lives on another context", fn);
    ORX_ARG(opt->kind == ORX_SGD || opt->kind == ORX_MOMENTUM || opt->kind == ORX_ADAGRAD || opt->kind == ORX_ADAM,
            "%s: unknown optimizer kind %d", fn, opt->kind);
    ORX_ARG(opt->kind != ORX_ADAM || opt->t + 1 < 0x7fffffff, "%s: step counter overflow", fn);
    ORX_HIP(hipSetDevice(c->device));
    CHECK(orx_table_sync(t));                              // (lazy under this or another optimizer: every row current first)
    if (opt->kind == ORX_ADAM) {
        CHECK(orx_opt_isolate(opt, &t, 1));                // (a shared optimizer: see orx_opt_isolate)
        opt->t += 1;
    }
    return orx_table_apply_dense_at(c, opt, t, grad);
}
