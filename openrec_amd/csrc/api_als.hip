// C-ABI entry points of alternating least squares for WRMF: orx_als_half_step, orx_als_segment_len (kernels_als.hip has the kernels
// and the design; include/openrec_hip.h the contract).
#include "orx_internal.h"

int orx_als_seg_len();
int64_t orx_als_slot_floats(int D);
int orx_als_gram_blocks(int64_t M);
int orx_launch_als(orx_ctx* ctx, const float* F, int64_t M, int D, float* X, const int64_t* rp, const int32_t* cols, const float* conf,
                   int64_t nrows, float a, float b, float reg, float* gram_part, float* Gm,
                   int cap, unsigned long long* counter, int* seg_base, int2* list, float* slots);

constexpr size_t ALS_SLOT_BUDGET = (size_t)1 << 30;      // most scratch the partials of long rows may take when only the device knows the CSR

extern "C" int32_t orx_als_segment_len(void) { return orx_als_seg_len(); }

static size_t als_up(size_t x) { return (x + 255) & ~(size_t)255; }

extern "C" int orx_als_half_step(orx_ctx* c, orx_table* fixed, orx_table* solved, const int64_t* row_ptr, const int32_t* cols,
                                 const float* conf, int64_t row0, int64_t nrows, float a, float b, float reg, int flags) {
    static const char* fn = "orx_als_half_step";
    ORX_ARG(c && fixed && solved, "%s: NULL context or table", fn);
    ORX_ARG(fixed != solved, "%s: the fixed and the solved table are the same table", fn);
    ORX_ARG(fixed->ctx == c && solved->ctx == c, "%s: the tables live on another context", fn);
    ORX_ARG(fixed->dim == solved->dim, "%s: fixed dim %d, solved dim %d", fn, fixed->dim, solved->dim);
    ORX_ARG(fixed->dim >= 1 && fixed->dim <= 128, "%s: dim %d outside [1, 128]", fn, fixed->dim);
    ORX_ARG((flags & ~ORX_IDS_DEVICE) == 0, "%s: unknown flags 0x%x", fn, flags);
    ORX_ARG(std::isfinite(reg) && reg > 0.f, "%s: reg must be finite and > 0, got %g", fn, (double)reg);
    ORX_ARG(b >= 0.f && std::isfinite(b), "%s: b must be finite and >= 0, got %g", fn, (double)b);
    ORX_ARG(conf || (a >= b && std::isfinite(a)), "%s: a = %g must be finite and >= b = %g", fn, (double)a, (double)b);
    ORX_ARG(row0 >= 0 && nrows >= 0 && row0 <= solved->rows && nrows <= solved->rows - row0,
            "%s: rows [%lld, %lld) outside the solved table's %lld rows", fn, (long long)row0, (long long)(row0 + nrows), (long long)solved->rows);
    if (nrows == 0) return ORX_OK;
    ORX_ARG(row_ptr, "%s: NULL row_ptr", fn);
    const bool dev = (flags & ORX_IDS_DEVICE) != 0;
    const int D = fixed->dim;
    const int64_t M = fixed->rows, L = orx_als_seg_len();
    const size_t slot_bytes = (size_t)orx_als_slot_floats(D) * sizeof(float);

    // how many scratch slots the segments of long rows may take
    int64_t e_first = 0, e_count = 0, cap = 0;
    if (!dev) {
        e_first = row_ptr[row0];
        ORX_ARG(e_first >= 0, "%s: row_ptr[%lld] is negative", fn, (long long)row0);
        for (int64_t i = 0; i < nrows; ++i) {
            const int64_t n = row_ptr[row0 + i + 1] - row_ptr[row0 + i];
            ORX_ARG(n >= 0, "%s: row_ptr decreases at row %lld", fn, (long long)(row0 + i));
            if (n > L) cap += (n + L - 1) / L;
        }
        e_count = row_ptr[row0 + nrows] - e_first;
        ORX_ARG(e_count == 0 || cols, "%s: NULL cols", fn);
    } else {
        ORX_ARG(cols, "%s: NULL cols", fn);
        if (M > L) {                                       // the columns of a row are distinct: none is longer than M
            const int64_t per_row = (M + L - 1) / L, budget = (int64_t)(ALS_SLOT_BUDGET / slot_bytes);
            cap = nrows < budget / per_row ? nrows * per_row : budget;
        }
    }
    const int64_t budget_all = (int64_t)1 << 24;           // the plan's slot numbers are ints
    if (cap > budget_all) cap = budget_all;

    // both tables as every reader sees them: a lazily-applied Adam is finished first (the solved rows are about to be overwritten,
    // steps still owed to them must not be replayed on top of the solution); optimizer slots are not touched
    CHECK(orx_table_sync(fixed));
    CHECK(orx_table_sync(solved));
    ORX_HIP(hipSetDevice(c->device));

    const int Dp = (D + 15) / 16 * 16;
    const int nb = orx_als_gram_blocks(M);
    ENSURE(c->d_tmp, c->d_tmp_cap, (size_t)(nb + 1) * Dp * Dp * sizeof(float));
    float* Gm = c->d_tmp; float* gram_part = c->d_tmp + (size_t)Dp * Dp;
    // d_topk: row offsets (host CSR) | counter | slot base per row | segment list
    const size_t o_rp = 0, o_cnt = o_rp + als_up(dev ? 0 : (size_t)(nrows + 1) * sizeof(int64_t)), o_base = o_cnt + 256,
                 o_list = o_base + als_up(cap ? (size_t)nrows * sizeof(int) : 0), total = o_list + als_up((size_t)cap * sizeof(int2));
    ENSURE(c->d_topk, c->d_topk_cap, total);
    if (cap) ENSURE(c->d_splitk, c->d_splitk_cap, (size_t)cap * slot_bytes);
    const int64_t* d_rp = row_ptr + row0;
    const int32_t* d_cols = cols;
    const float* d_conf = conf;
    if (!dev) {
        std::vector<int64_t> rp((size_t)nrows + 1);
        for (int64_t i = 0; i <= nrows; ++i) rp[(size_t)i] = row_ptr[row0 + i] - e_first;      // entry 0 = the first staged entry
        int64_t* drp = reinterpret_cast<int64_t*>(c->d_topk + o_rp);
        ORX_HIP(hipMemcpyAsync(drp, rp.data(), rp.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        ENSURE(c->d_ids, c->d_ids_cap, (size_t)(e_count ? e_count : 1) * sizeof(int32_t));
        if (e_count) ORX_HIP(hipMemcpyAsync(c->d_ids, cols + e_first, (size_t)e_count * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        if (conf) {
            ENSURE(c->d_lab, c->d_lab_cap, (size_t)(e_count ? e_count : 1) * sizeof(float));
            if (e_count) ORX_HIP(hipMemcpyAsync(c->d_lab, conf + e_first, (size_t)e_count * sizeof(float), hipMemcpyHostToDevice, c->stream));
            d_conf = c->d_lab;
        }
        ORX_HIP(hipStreamSynchronize(c->stream));          // `rp` is a local: its copy must have left before it goes
        d_rp = drp; d_cols = c->d_ids;
    }
    CHECK(orx_launch_als(c, fixed->w, M, D, solved->w + (size_t)row0 * D, d_rp, d_cols, d_conf, nrows, a, b, reg, gram_part, Gm, (int)cap,
                         reinterpret_cast<unsigned long long*>(c->d_topk + o_cnt), reinterpret_cast<int*>(c->d_topk + o_base),
                         reinterpret_cast<int2*>(c->d_topk + o_list), c->d_splitk));
    solved->version++;
    if (!dev) return orx_check_index_error(c);
    return ORX_OK;
}
