// C-ABI entry points of the conjugate-gradient ALS half-step and of the ALS objective: orx_als_half_step_cg,
// orx_als_cg_row_breaks, orx_als_objective (kernels_als_cg.hip has the kernels and the design; include/openrec_hip.h the contract).
// The argument rules are orx_als_half_step's (api_als.hip), restated here so that the Cholesky path stays as it is.
#include "orx_als_cg.h"

constexpr int64_t CG_SLOT_CAP = (int64_t)1 << 16;      // most scratch slots the segments of a call's long rows may take

// ORX_ALS_CG_SLOTS (read per call) lowers that budget: rows that get no slots are walked by one wavefront -- the same bits (tests)
static int64_t cg_slot_cap() {
    const char* e = getenv("ORX_ALS_CG_SLOTS");
    if (e && *e) {
        const long long v = atoll(e);
        if (v >= 0 && v < CG_SLOT_CAP) return v;
    }
    return CG_SLOT_CAP;
}

extern "C" int32_t orx_als_cg_row_breaks(int32_t dim, int32_t* out, int32_t cap) { return orx_als_cg_breaks(dim, out, out ? cap : 0); }

static size_t cg_up(size_t x) { return (x + 255) & ~(size_t)255; }

// what both entry points ask of (tables, scalars, flags)
static int cg_check(const char* fn, orx_ctx* c, orx_table* fixed, orx_table* solved, const float* conf, float a, float b, float reg, int flags) {
    ORX_ARG(c && fixed && solved, "%s: NULL context or table", fn);
    ORX_ARG(fixed != solved, "%s: the two tables are the same table", fn);
    ORX_ARG(fixed->ctx == c && solved->ctx == c, "%s: the tables live on another context", fn);
    ORX_ARG(fixed->dim == solved->dim, "%s: dims %d and %d", fn, fixed->dim, solved->dim);
    ORX_ARG(fixed->dim >= 1 && fixed->dim <= 128, "%s: dim %d outside [1, 128]", fn, fixed->dim);
    ORX_ARG((flags & ~ORX_IDS_DEVICE) == 0, "%s: unknown flags 0x%x", fn, flags);
    ORX_ARG(std::isfinite(reg) && reg > 0.f, "%s: reg must be finite and > 0, got %g", fn, (double)reg);
    ORX_ARG(b >= 0.f && std::isfinite(b), "%s: b must be finite and >= 0, got %g", fn, (double)b);
    ORX_ARG(conf || (a >= b && std::isfinite(a)), "%s: a = %g must be finite and >= b = %g", fn, (double)a, (double)b);
    return ORX_OK;
}

// rows [row0, row0 + nrows) of a host CSR onto the device (row offsets rebased to the first staged entry): d_topk + o_rp, d_ids, d_lab
static int cg_stage(const char* fn, orx_ctx* c, const int64_t* row_ptr, const int32_t* cols, const float* conf, int64_t row0, int64_t nrows,
                    size_t o_rp, const int64_t** d_rp, const int32_t** d_cols, const float** d_conf) {
    const int64_t e_first = row_ptr[row0], e_count = row_ptr[row0 + nrows] - e_first;
    std::vector<int64_t> rp((size_t)nrows + 1);
    for (int64_t i = 0; i <= nrows; ++i) rp[(size_t)i] = row_ptr[row0 + i] - e_first;
    int64_t* drp = reinterpret_cast<int64_t*>(c->d_topk + o_rp);
    ORX_HIP(hipMemcpyAsync(drp, rp.data(), rp.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    ENSURE(c->d_ids, c->d_ids_cap, (size_t)(e_count ? e_count : 1) * sizeof(int32_t));
    if (e_count) ORX_HIP(hipMemcpyAsync(c->d_ids, cols + e_first, (size_t)e_count * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    *d_conf = nullptr;
    if (conf) {
        ENSURE(c->d_lab, c->d_lab_cap, (size_t)(e_count ? e_count : 1) * sizeof(float));
        if (e_count) ORX_HIP(hipMemcpyAsync(c->d_lab, conf + e_first, (size_t)e_count * sizeof(float), hipMemcpyHostToDevice, c->stream));
        *d_conf = c->d_lab;
    }
    ORX_HIP(hipStreamSynchronize(c->stream));              // `rp` is a local: its copy must have left before it goes
    *d_rp = drp; *d_cols = c->d_ids;
    (void)fn;
    return ORX_OK;
}

extern "C" int orx_als_half_step_cg(orx_ctx* c, orx_table* fixed, orx_table* solved, const int64_t* row_ptr, const int32_t* cols,
                                    const float* conf, int64_t row0, int64_t nrows, float a, float b, float reg, int32_t cg_steps, int flags) {
    static const char* fn = "orx_als_half_step_cg";
    CHECK(cg_check(fn, c, fixed, solved, conf, a, b, reg, flags));
    ORX_ARG(cg_steps >= 1 && cg_steps <= 128, "%s: cg_steps %d outside [1, 128]", fn, cg_steps);
    ORX_ARG(row0 >= 0 && nrows >= 0 && row0 <= solved->rows && nrows <= solved->rows - row0,
            "%s: rows [%lld, %lld) outside the solved table's %lld rows", fn, (long long)row0, (long long)(row0 + nrows), (long long)solved->rows);
    if (nrows == 0) return ORX_OK;
    ORX_ARG(row_ptr, "%s: NULL row_ptr", fn);
    const bool dev = (flags & ORX_IDS_DEVICE) != 0;
    const int D = fixed->dim;
    const int64_t M = fixed->rows, L = orx_als_cg_seg();

    // state slots (one per long row) and scratch slots (one per segment of a long row)
    int64_t cap_rows = 0, cap_slots = 0;
    if (!dev) {
        ORX_ARG(row_ptr[row0] >= 0, "%s: row_ptr[%lld] is negative", fn, (long long)row0);
        for (int64_t i = 0; i < nrows; ++i) {
            const int64_t n = row_ptr[row0 + i + 1] - row_ptr[row0 + i];
            ORX_ARG(n >= 0, "%s: row_ptr decreases at row %lld", fn, (long long)(row0 + i));
            if (n > L) { cap_rows++; cap_slots += (n + L - 1) / L; }
        }
        ORX_ARG(row_ptr[row0 + nrows] == row_ptr[row0] || cols, "%s: NULL cols", fn);
    } else {
        ORX_ARG(cols, "%s: NULL cols", fn);
        if (M > L) {                                       // the columns of a row are distinct: none is longer than M
            const int64_t per_row = (M + L - 1) / L;
            cap_slots = nrows < CG_SLOT_CAP / per_row ? nrows * per_row : CG_SLOT_CAP;
            cap_rows = cap_slots / 2 < nrows ? cap_slots / 2 : nrows;      // a long row has at least two segments
        }
    }
    const int64_t budget = cg_slot_cap();
    if (cap_slots > budget) cap_slots = budget;
    if (cap_rows > cap_slots) cap_rows = cap_slots;

    CHECK(orx_table_sync(fixed));
    CHECK(orx_table_sync(solved));
    ORX_HIP(hipSetDevice(c->device));

    const int Dp16 = (D + 15) / 16 * 16, Dp = D <= 64 ? 64 : 128;
    const int nb = orx_als_gram_blocks(M);
    // d_tmp: Gm | Gq | the gram's slab partials
    ENSURE(c->d_tmp, c->d_tmp_cap, ((size_t)(nb + 1) * Dp16 * Dp16 + (size_t)orx_als_cg_square_floats(D)) * sizeof(float));
    float* Gm = c->d_tmp; float* Gq = Gm + (size_t)Dp16 * Dp16; float* gram_part = Gq + (size_t)orx_als_cg_square_floats(D);
    // d_topk: row offsets (host CSR) | counter | state slot per row | row list | segment list | x | r | rs | p
    const size_t o_rp = 0, o_cnt = o_rp + cg_up(dev ? 0 : (size_t)(nrows + 1) * sizeof(int64_t)), o_idx = o_cnt + 256,
                 o_rows = o_idx + cg_up(cap_slots ? (size_t)nrows * sizeof(int) : 0), o_list = o_rows + cg_up((size_t)cap_rows * sizeof(int2)),
                 o_x = o_list + cg_up((size_t)cap_slots * sizeof(int2)), o_r = o_x + cg_up((size_t)cap_rows * Dp * sizeof(double)),
                 o_rs = o_r + cg_up((size_t)cap_rows * Dp * sizeof(double)), o_p = o_rs + cg_up((size_t)cap_rows * sizeof(double)),
                 total = o_p + cg_up((size_t)cap_rows * Dp * sizeof(float));
    ENSURE(c->d_topk, c->d_topk_cap, total);
    if (cap_slots) ENSURE(c->d_splitk, c->d_splitk_cap, (size_t)cap_slots * orx_als_cg_slot_floats(D) * sizeof(float));
    CgArgs p;
    p.F = fixed->w; p.M = M; p.D = D; p.Gq = Gq; p.X = solved->w + (size_t)row0 * D;
    p.rp = row_ptr + row0; p.cols = cols; p.conf = conf;
    if (!dev) CHECK(cg_stage(fn, c, row_ptr, cols, conf, row0, nrows, o_rp, &p.rp, &p.cols, &p.conf));
    p.nrows = nrows; p.a = a; p.b = b; p.reg = reg; p.cg_steps = cg_steps;
    p.cap_rows = (int)cap_rows; p.cap_slots = (int)cap_slots; p.slots = c->d_splitk;
    p.sx = reinterpret_cast<double*>(c->d_topk + o_x); p.sr = reinterpret_cast<double*>(c->d_topk + o_r);
    p.srs = reinterpret_cast<double*>(c->d_topk + o_rs); p.sp = reinterpret_cast<float*>(c->d_topk + o_p);
    CHECK(orx_launch_als_gram(c, fixed->w, M, D, gram_part, Gm));
    CHECK(orx_launch_als_cg(c, p, Gm, Gq, reinterpret_cast<unsigned long long*>(c->d_topk + o_cnt), reinterpret_cast<int*>(c->d_topk + o_idx),
                            reinterpret_cast<int2*>(c->d_topk + o_rows), reinterpret_cast<int2*>(c->d_topk + o_list)));
    solved->version++;
    if (!dev) return orx_check_index_error(c);
    return ORX_OK;
}

extern "C" int orx_als_objective(orx_ctx* c, orx_table* user, orx_table* item, const int64_t* row_ptr, const int32_t* cols, const float* conf,
                                 float a, float b, float reg, int flags, double* host_out) {
    static const char* fn = "orx_als_objective";
    CHECK(cg_check(fn, c, item, user, conf, a, b, reg, flags));
    ORX_ARG(host_out, "%s: NULL host_out", fn);
    ORX_ARG(row_ptr, "%s: NULL row_ptr", fn);
    const bool dev = (flags & ORX_IDS_DEVICE) != 0;
    const int D = user->dim;
    const int64_t NU = user->rows, NI = item->rows;
    CHECK(orx_table_sync(user));
    CHECK(orx_table_sync(item));
    ORX_HIP(hipSetDevice(c->device));
    int64_t nnz = 0;
    if (!dev) {
        ORX_ARG(row_ptr[0] == 0, "%s: row_ptr[0] = %lld", fn, (long long)row_ptr[0]);
        for (int64_t i = 0; i < NU; ++i) ORX_ARG(row_ptr[i + 1] >= row_ptr[i], "%s: row_ptr decreases at row %lld", fn, (long long)i);
        nnz = row_ptr[NU];
    } else {
        ORX_HIP(hipMemcpyAsync(&nnz, row_ptr + NU, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        ORX_HIP(hipStreamSynchronize(c->stream));
        ORX_ARG(nnz >= 0, "%s: row_ptr ends at %lld", fn, (long long)nnz);
    }
    ORX_ARG(nnz == 0 || cols, "%s: NULL cols", fn);
    const int Dp16 = (D + 15) / 16 * 16;
    const int nbU = orx_als_gram_blocks(NU), nbV = orx_als_gram_blocks(NI);
    ObjArgs p;
    p.U = user->w; p.V = item->w; p.NU = NU; p.NI = NI; p.D = D; p.nnz = nnz; p.a = a; p.b = b; p.reg = reg;
    p.nw = orx_als_obj_waves(nnz); p.nbU = nbU; p.nbV = nbV; p.Dp16 = Dp16;
    ENSURE(c->d_tmp, c->d_tmp_cap, (size_t)(nbU + nbV) * Dp16 * Dp16 * sizeof(float));
    float* gU = c->d_tmp; float* gV = gU + (size_t)nbU * Dp16 * Dp16;
    p.ngw = orx_als_obj_gram_groups(D);
    // d_topk: row offsets (host CSR) | the result | the gram pass' partials | one partial per wavefront
    const size_t o_rp = 0, o_out = o_rp + cg_up(dev ? 0 : (size_t)(NU + 1) * sizeof(int64_t)), o_g = o_out + 256,
                 o_part = o_g + cg_up((size_t)p.ngw * 2 * sizeof(double)),
                 total = o_part + cg_up((size_t)p.nw * sizeof(double));
    ENSURE(c->d_topk, c->d_topk_cap, total);
    p.rp = row_ptr; p.cols = cols; p.conf = conf;
    if (!dev) CHECK(cg_stage(fn, c, row_ptr, cols, conf, 0, NU, o_rp, &p.rp, &p.cols, &p.conf));
    p.gramU = gU; p.gramV = gV; p.out = reinterpret_cast<double*>(c->d_topk + o_out); p.part = reinterpret_cast<double*>(c->d_topk + o_part);
    p.gpart = reinterpret_cast<double*>(c->d_topk + o_g);
    CHECK(orx_launch_als_gram(c, user->w, NU, D, gU, nullptr));
    CHECK(orx_launch_als_gram(c, item->w, NI, D, gV, nullptr));
    CHECK(orx_launch_als_objective(c, p));
    ORX_HIP(hipMemcpyAsync(host_out, p.out, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ORX_HIP(hipStreamSynchronize(c->stream));
    if (!dev) return orx_check_index_error(c);
    return ORX_OK;
}
