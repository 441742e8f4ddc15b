// The host driver of the calls that walk a row range of a CSR against a table, and their C-ABI entry points: orx_als_half_step,
// orx_als_half_step_cg, orx_als_objective (kernels_als.hip, kernels_als_cg.hip), orx_graph_spmm (kernels_graph.hip), and the
// geometry queries orx_als_segment_len, orx_graph_segment_len, orx_als_cg_row_breaks.  include/openrec_hip.h has the contract,
// DESIGN.md 4.5t what the driver provides and what a call keeps to itself.  No kernel is defined or instantiated here: orx_seg_plan.h comes in
// through the two headers for SegScratch alone.
#include <algorithm>

#include "orx_als.h"
#include "orx_graph.h"

extern "C" int32_t orx_als_segment_len(void) { return ALS_SEG; }
extern "C" int32_t orx_graph_segment_len(void) { return GS_SEG; }
extern "C" int32_t orx_als_cg_row_breaks(int32_t dim, int32_t* out, int32_t cap) { return orx_als_cg_breaks(dim, out, out ? cap : 0); }

// ---- argument checks -------------------------------------------------------------------------------------------------------
// what the ALS calls ask of (tables, scalars, flags)
static int csr_check_als(const char* fn, orx_ctx* c, orx_table* fixed, orx_table* solved, const float* conf, float a, float b, float reg, int flags) {
    ORX_ARG(c && fixed && solved, "%s: NULL context or table", fn);
    ORX_ARG(fixed != solved, "%s: the fixed and the solved table are the same table", fn);
    ORX_ARG(fixed->ctx == c && solved->ctx == c, "%s: the tables live on another context", fn);
    ORX_ARG(fixed->dim == solved->dim, "%s: fixed dim %d, solved dim %d", fn, fixed->dim, solved->dim);
    ORX_ARG(fixed->dim >= 1 && fixed->dim <= 128, "%s: dim %d outside [1, 128]", fn, fixed->dim);
    ORX_ARG((flags & ~ORX_IDS_DEVICE) == 0, "%s: unknown flags 0x%x", fn, flags);
    ORX_ARG(std::isfinite(reg) && reg > 0.f, "%s: reg must be finite and > 0, got %g", fn, (double)reg);
    ORX_ARG(b >= 0.f && std::isfinite(b), "%s: b must be finite and >= 0, got %g", fn, (double)b);
    ORX_ARG(conf || (a >= b && std::isfinite(a)), "%s: a = %g must be finite and >= b = %g", fn, (double)a, (double)b);
    return ORX_OK;
}

// rows [row0, row0 + nrows) lie inside the table the call writes (`what` names it)
static int csr_check_rows(const char* fn, const char* what, int64_t table_rows, int64_t row0, int64_t nrows) {
    ORX_ARG(row0 >= 0 && nrows >= 0 && row0 <= table_rows && nrows <= table_rows - row0,
            "%s: rows [%lld, %lld) outside %s's %lld rows", fn, (long long)row0, (long long)(row0 + nrows), what, (long long)table_rows);
    return ORX_OK;
}

// The CSR of nrows > 0 rows.  A host CSR: offsets that start at >= 0 and never decrease, cols unless the range has no entry; ->
// the rows of more than `seg` entries and the segments they are cut into.  A device CSR: cols, nothing is read.
static int csr_scan(const char* fn, const int64_t* row_ptr, const int32_t* cols, int64_t row0, int64_t nrows, bool dev, int64_t seg,
                    int64_t* long_rows, int64_t* segments) {
    *long_rows = *segments = 0;
    ORX_ARG(row_ptr, "%s: NULL row_ptr", fn);
    if (dev) { ORX_ARG(cols, "%s: NULL cols", fn); return ORX_OK; }
    ORX_ARG(row_ptr[row0] >= 0, "%s: row_ptr[%lld] is negative", fn, (long long)row0);
    for (int64_t i = 0; i < nrows; ++i) {
        const int64_t n = row_ptr[row0 + i + 1] - row_ptr[row0 + i];
        ORX_ARG(n >= 0, "%s: row_ptr decreases at row %lld", fn, (long long)(row0 + i));
        if (n > seg) { ++*long_rows; *segments += (n + seg - 1) / seg; }
    }
    ORX_ARG(row_ptr[row0 + nrows] == row_ptr[row0] || cols, "%s: NULL cols", fn);
    return ORX_OK;
}

// ---- scratch slots of the long rows --------------------------------------------------------------------------------------------
// Most scratch the segments of a call's long rows may take when only the device knows the CSR (bytes: the slot's size is the
// call's), most slots of a CG call wherever its CSR lives, and what every plan stops at: its slot numbers are ints.
constexpr int64_t ALS_SLOT_BYTES = (int64_t)1 << 30, GRAPH_SLOT_BYTES = (int64_t)1 << 28, CG_SLOT_CAP = (int64_t)1 << 16,
                  PLAN_SLOT_CAP = (int64_t)1 << 24;

// a device CSR: the columns of a row are distinct, so no row is longer than M
static int64_t csr_device_bound(int64_t M, int64_t seg, int64_t nrows, int64_t budget_slots) {
    if (M <= seg) return 0;
    const int64_t per_row = (M + seg - 1) / seg;
    return nrows < budget_slots / per_row ? nrows * per_row : budget_slots;
}

// ORX_ALS_CG_SLOTS (read per call) lowers the CG budget: rows that get no slots are walked by one wavefront -- the same bits (tests)
static int64_t cg_slot_cap() {
    const char* e = getenv("ORX_ALS_CG_SLOTS");
    if (e && *e) {
        const long long v = atoll(e);
        if (v >= 0 && v < CG_SLOT_CAP) return v;
    }
    return CG_SLOT_CAP;
}

// ---- staging, scratch, tail ------------------------------------------------------------------------------------------------------
// rows [row0, row0 + nrows) of a host CSR onto the device: the offsets, rebased to the first staged entry, into d_rp; the columns
// into d_ids; the confidences into d_lab (conf NULL: nothing is copied and *dconf is left as the caller set it, which is conf).
// d_ids is sized before the first copy; the copies go offsets, columns, confidences.  Synchronises: the rebased offsets are a local.
static int csr_stage(orx_ctx* c, const int64_t* row_ptr, const int32_t* cols, const float* conf, int64_t row0, int64_t nrows, int64_t* d_rp,
                     const int64_t** rp, const int32_t** dcols, const float** dconf) {
    const int64_t count = row_ptr[row0 + nrows] - row_ptr[row0];
    std::vector<int64_t> hp((size_t)nrows + 1);
    CsrSlice s;
    ENSURE(c->d_ids, c->d_ids_cap, (size_t)(count ? count : 1) * sizeof(int32_t));
    CHECK(orx_stage_csr(c, row_ptr, cols, row0, nrows, hp.data(), nullptr, d_rp, c->d_ids, &s));
    if (conf) {
        ENSURE(c->d_lab, c->d_lab_cap, (size_t)(count ? count : 1) * sizeof(float));
        if (count) ORX_HIP(hipMemcpyAsync(c->d_lab, conf + s.first, (size_t)count * sizeof(float), hipMemcpyHostToDevice, c->stream));
        *dconf = c->d_lab;
    }
    ORX_HIP(hipStreamSynchronize(c->stream));
    *rp = d_rp; *dcols = c->d_ids;
    return ORX_OK;
}

// the scratch of a Cholesky or graph plan of `cap` slots.  d_topk: row offsets (host CSR) | counter | slot base per row | segment
// list; d_splitk: the slots
static int csr_seg_scratch(orx_ctx* c, bool dev, int64_t nrows, int64_t cap, size_t slot_bytes, int64_t** d_rp, SegScratch* s) {
    Carve cv;
    const size_t o_rp = cv.take(dev ? 0 : (size_t)(nrows + 1) * sizeof(int64_t)), o_cnt = cv.take(256),
                 o_base = cv.take(cap ? (size_t)nrows * sizeof(int) : 0), o_list = cv.take((size_t)cap * sizeof(int2));
    ENSURE(c->d_topk, c->d_topk_cap, cv.off);
    if (cap) ENSURE(c->d_splitk, c->d_splitk_cap, (size_t)cap * slot_bytes);
    *d_rp = reinterpret_cast<int64_t*>(c->d_topk + o_rp);
    *s = SegScratch{(int)cap, reinterpret_cast<unsigned long long*>(c->d_topk + o_cnt), reinterpret_cast<int*>(c->d_topk + o_base),
                    reinterpret_cast<int2*>(c->d_topk + o_list), c->d_splitk};
    return ORX_OK;
}

// after the launches: the tables written are another version; a host CSR's columns were checked by the kernels
static int csr_done(orx_ctx* c, bool dev, std::initializer_list<orx_table*> written) {
    for (orx_table* t : written) if (t) t->version++;
    return dev ? ORX_OK : orx_check_index_error(c);
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
extern "C" int orx_als_half_step(orx_ctx* c, orx_table* fixed, orx_table* solved, const int64_t* row_ptr, const int32_t* cols,
                                 const float* conf, int64_t row0, int64_t nrows, float a, float b, float reg, int flags) {
    static const char* fn = "orx_als_half_step";
    CHECK(csr_check_als(fn, c, fixed, solved, conf, a, b, reg, flags));
    CHECK(csr_check_rows(fn, "the solved table", solved->rows, row0, nrows));
    if (nrows == 0) return ORX_OK;
    const bool dev = (flags & ORX_IDS_DEVICE) != 0;
    const int D = fixed->dim;
    const int64_t M = fixed->rows;
    const size_t slot_bytes = (size_t)orx_als_slot_floats(D) * sizeof(float);
    int64_t long_rows, cap;
    CHECK(csr_scan(fn, row_ptr, cols, row0, nrows, dev, ALS_SEG, &long_rows, &cap));
    if (dev) cap = csr_device_bound(M, ALS_SEG, nrows, ALS_SLOT_BYTES / (int64_t)slot_bytes);
    cap = std::min(cap, PLAN_SLOT_CAP);

    // both tables as every reader sees them: a lazily-applied Adam is finished first (the solved rows are about to be overwritten,
    // steps still owed to them must not be replayed on top of the solution); optimizer slots are not touched
    CHECK(orx_table_sync(fixed));
    CHECK(orx_table_sync(solved));
    ORX_HIP(hipSetDevice(c->device));

    const int Dp = (D + 15) / 16 * 16;
    ENSURE(c->d_tmp, c->d_tmp_cap, (size_t)(orx_als_gram_blocks(M) + 1) * Dp * Dp * sizeof(float));
    float* Gm = c->d_tmp; float* gram_part = c->d_tmp + (size_t)Dp * Dp;
    int64_t* d_rp; SegScratch s;
    CHECK(csr_seg_scratch(c, dev, nrows, cap, slot_bytes, &d_rp, &s));
    const int64_t* rp = row_ptr + row0;
    if (!dev) CHECK(csr_stage(c, row_ptr, cols, conf, row0, nrows, d_rp, &rp, &cols, &conf));
    CHECK(orx_launch_als_gram(c, fixed->w, M, D, gram_part, Gm));
    CHECK(orx_launch_als(c, fixed->w, M, D, solved->w + (size_t)row0 * D, rp, cols, conf, nrows, a, b, reg, Gm, s));
    return csr_done(c, dev, {solved});
}

extern "C" int orx_als_half_step_cg(orx_ctx* c, orx_table* fixed, orx_table* solved, const int64_t* row_ptr, const int32_t* cols,
                                    const float* conf, int64_t row0, int64_t nrows, float a, float b, float reg, int32_t cg_steps, int flags) {
    static const char* fn = "orx_als_half_step_cg";
    CHECK(csr_check_als(fn, c, fixed, solved, conf, a, b, reg, flags));
    ORX_ARG(cg_steps >= 1 && cg_steps <= 128, "%s: cg_steps %d outside [1, 128]", fn, cg_steps);
    CHECK(csr_check_rows(fn, "the solved table", solved->rows, row0, nrows));
    if (nrows == 0) return ORX_OK;
    const bool dev = (flags & ORX_IDS_DEVICE) != 0;
    const int D = fixed->dim;
    const int64_t M = fixed->rows;
    // state slots (one per long row) and scratch slots (one per segment of a long row)
    int64_t cap_rows, cap_slots;
    CHECK(csr_scan(fn, row_ptr, cols, row0, nrows, dev, ALS_SEG, &cap_rows, &cap_slots));
    if (dev) {
        cap_slots = csr_device_bound(M, ALS_SEG, nrows, CG_SLOT_CAP);
        cap_rows = std::min(cap_slots / 2, nrows);         // a long row has at least two segments
    }
    cap_slots = std::min(cap_slots, cg_slot_cap());
    cap_rows = std::min(cap_rows, cap_slots);

    CHECK(orx_table_sync(fixed));
    CHECK(orx_table_sync(solved));
    ORX_HIP(hipSetDevice(c->device));

    const int Dp16 = (D + 15) / 16 * 16, Dp = D <= 64 ? 64 : 128;
    // d_tmp: Gm | Gq | the gram's slab partials
    ENSURE(c->d_tmp, c->d_tmp_cap, ((size_t)(orx_als_gram_blocks(M) + 1) * Dp16 * Dp16 + (size_t)orx_als_cg_square_floats(D)) * sizeof(float));
    float* Gm = c->d_tmp; float* Gq = Gm + (size_t)Dp16 * Dp16; float* gram_part = Gq + (size_t)orx_als_cg_square_floats(D);
    // d_topk: row offsets (host CSR) | counter | state slot per row | row list | segment list | x | r | rs | p
    Carve cv;
    const size_t o_rp = cv.take(dev ? 0 : (size_t)(nrows + 1) * sizeof(int64_t)), o_cnt = cv.take(256),
                 o_idx = cv.take(cap_slots ? (size_t)nrows * sizeof(int) : 0), o_rows = cv.take((size_t)cap_rows * sizeof(int2)),
                 o_list = cv.take((size_t)cap_slots * sizeof(int2)), o_x = cv.take((size_t)cap_rows * Dp * sizeof(double)),
                 o_r = cv.take((size_t)cap_rows * Dp * sizeof(double)), o_rs = cv.take((size_t)cap_rows * sizeof(double)),
                 o_p = cv.take((size_t)cap_rows * Dp * sizeof(float));
    ENSURE(c->d_topk, c->d_topk_cap, cv.off);
    if (cap_slots) ENSURE(c->d_splitk, c->d_splitk_cap, (size_t)cap_slots * orx_als_cg_slot_floats(D) * sizeof(float));
    CgArgs p;
    p.F = fixed->w; p.M = M; p.D = D; p.Gq = Gq; p.X = solved->w + (size_t)row0 * D;
    p.rp = row_ptr + row0; p.cols = cols; p.conf = conf;
    if (!dev) CHECK(csr_stage(c, row_ptr, cols, conf, row0, nrows, reinterpret_cast<int64_t*>(c->d_topk + o_rp), &p.rp, &p.cols, &p.conf));
    p.nrows = nrows; p.a = a; p.b = b; p.reg = reg; p.cg_steps = cg_steps;
    p.cap_rows = (int)cap_rows; p.cap_slots = (int)cap_slots; p.slots = c->d_splitk;
    p.sx = reinterpret_cast<double*>(c->d_topk + o_x); p.sr = reinterpret_cast<double*>(c->d_topk + o_r);
    p.srs = reinterpret_cast<double*>(c->d_topk + o_rs); p.sp = reinterpret_cast<float*>(c->d_topk + o_p);
    CHECK(orx_launch_als_gram(c, fixed->w, M, D, gram_part, Gm));
    CHECK(orx_launch_als_cg(c, p, Gm, Gq, reinterpret_cast<unsigned long long*>(c->d_topk + o_cnt), reinterpret_cast<int*>(c->d_topk + o_idx),
                            reinterpret_cast<int2*>(c->d_topk + o_rows), reinterpret_cast<int2*>(c->d_topk + o_list)));
    return csr_done(c, dev, {solved});
}

// the whole CSR, not a row range: its own rule (offsets from 0; a device CSR's nnz is read back)
extern "C" int orx_als_objective(orx_ctx* c, orx_table* user, orx_table* item, const int64_t* row_ptr, const int32_t* cols, const float* conf,
                                 float a, float b, float reg, int flags, double* host_out) {
    static const char* fn = "orx_als_objective";
    CHECK(csr_check_als(fn, c, item, user, conf, a, b, reg, flags));
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
    Carve cv;
    const size_t o_rp = cv.take(dev ? 0 : (size_t)(NU + 1) * sizeof(int64_t)), o_out = cv.take(256),
                 o_g = cv.take((size_t)p.ngw * 2 * sizeof(double)), o_part = cv.take((size_t)p.nw * sizeof(double));
    ENSURE(c->d_topk, c->d_topk_cap, cv.off);
    p.rp = row_ptr; p.cols = cols; p.conf = conf;
    if (!dev) CHECK(csr_stage(c, row_ptr, cols, conf, 0, NU, reinterpret_cast<int64_t*>(c->d_topk + o_rp), &p.rp, &p.cols, &p.conf));
    p.gramU = gU; p.gramV = gV; p.out = reinterpret_cast<double*>(c->d_topk + o_out); p.part = reinterpret_cast<double*>(c->d_topk + o_part);
    p.gpart = reinterpret_cast<double*>(c->d_topk + o_g);
    CHECK(orx_launch_als_gram(c, user->w, NU, D, gU, nullptr));
    CHECK(orx_launch_als_gram(c, item->w, NI, D, gV, nullptr));
    CHECK(orx_launch_als_objective(c, p));
    ORX_HIP(hipMemcpyAsync(host_out, p.out, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ORX_HIP(hipStreamSynchronize(c->stream));
    return csr_done(c, dev, {});
}

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
    CHECK(csr_check_rows(fn, "out", out->rows, row0, nrows));
    if (nrows == 0) return ORX_OK;
    const bool dev = (flags & ORX_IDS_DEVICE) != 0;
    const int D = X->dim;
    const int64_t M = X->rows;
    const size_t slot_bytes = (size_t)D * sizeof(float);
    int64_t long_rows, cap;
    CHECK(csr_scan(fn, row_ptr, cols, row0, nrows, dev, GS_SEG, &long_rows, &cap));
    if (dev) {
        // long_segments >= 0: the caller counted the segments of the CSR's rows of more than GS_SEG entries once (an upper bound for
        // any row range; 0: no plan, no segment launch, no scratch).  A count that is too small costs nothing but time: rows that
        // find no slot walk their segments themselves.  < 0: unknown
        const int64_t budget = GRAPH_SLOT_BYTES / (int64_t)slot_bytes;
        cap = long_segments >= 0 ? std::min(long_segments, budget) : csr_device_bound(M, GS_SEG, nrows, budget);
    }
    cap = std::min(cap, PLAN_SLOT_CAP);

    // the tables as every reader sees them: a lazily-applied Adam is finished first
    CHECK(orx_table_sync(X));
    CHECK(orx_table_sync(out));
    if (acc) CHECK(orx_table_sync(acc));
    ORX_HIP(hipSetDevice(c->device));

    int64_t* d_rp; SegScratch s;
    CHECK(csr_seg_scratch(c, dev, nrows, cap, slot_bytes, &d_rp, &s));
    const int64_t* rp = row_ptr + row0;
    const float* no_conf = nullptr;
    if (!dev) CHECK(csr_stage(c, row_ptr, cols, nullptr, row0, nrows, d_rp, &rp, &cols, &no_conf));
    const bool vec_ok = D % 4 == 0 && (uintptr_t)X->w % 16 == 0 && (uintptr_t)out->w % 16 == 0 && (!acc || (uintptr_t)acc->w % 16 == 0) &&
                        (uintptr_t)c->d_splitk % 16 == 0;
    CHECK(orx_launch_graph_spmm(c, X->w, M, D, out->w + (size_t)row0 * D, acc ? acc->w + (size_t)row0 * D : nullptr, acc_alpha, rp, cols,
                                row_scale ? row_scale + row0 : nullptr, col_scale, nrows, vec_ok, s));
    return csr_done(c, dev, {out, acc});
}
