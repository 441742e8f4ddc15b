// Internal declarations shared by the translation units of libopenrec_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cmath>
#include <cstdarg>
#include <functional>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/openrec_hip.h"

// ---------------------------------------------------------------- errors ---
void orx_set_error(const char* fmt, ...);

#define ORX_HIP(expr)                                                                  \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess) {                                                        \
            orx_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),       \
                          __FILE__, __LINE__);                                         \
            return _e == hipErrorOutOfMemory ? ORX_ERR_OOM : ORX_ERR_HIP;              \
        }                                                                              \
    } while (0)

#define ORX_ARG(cond, ...)                                                             \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            orx_set_error(__VA_ARGS__);                                                \
            return ORX_ERR_ARG;                                                        \
        }                                                                              \
    } while (0)

// inside a function that returns an orx status: pass a failed call's status on / grow a device buffer (orx_ensure)
#define CHECK(call)                                                                    \
    do {                                                                               \
        int _rc = (call);                                                              \
        if (_rc != ORX_OK) return _rc;                                                 \
    } while (0)

#define ENSURE(ptr, cap, bytes)                                                        \
    do {                                                                               \
        int _rc = orx_ensure((void**)&(ptr), &(cap), (bytes));                         \
        if (_rc != ORX_OK) return _rc;                                                 \
    } while (0)

// --------------------------------------------------------------- objects ---
struct ProfSlot {
    std::vector<hipEvent_t> ev;   // pairs (start, stop) awaiting collection
    double total_ms = 0.0;
    int64_t launches = 0;
};

struct orx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int* d_err = nullptr;             // sticky device-side "id out of range" flag
    std::vector<struct orx_opt*> opts;  // live optimizers: a table that is destroyed takes its slots out of them
    // staging buffers (grown on demand)
    int32_t* d_ids = nullptr;  size_t d_ids_cap = 0;       // host-id upload
    float* d_lab = nullptr;    size_t d_lab_cap = 0;
    unsigned* d_evalbits = nullptr; size_t d_evalbits_cap = 0;  // evaluation bitmaps (orx_rank_metrics_csr): all zero between calls
    unsigned char* d_dflag = nullptr; size_t d_dflag_cap = 0;   // [K][2B] duplicate flags (pointwise, censor)
    int32_t* d_ids2 = nullptr; size_t d_ids2_cap = 0;            // [K][3B] ids with the duplicate flag in bit 31
    unsigned char* d_roles = nullptr; size_t d_roles_cap = 0;    // [K][3B] dedup scratch
    unsigned char* d_cflag = nullptr; size_t d_cflag_cap = 0;    // [3][K][B] censor election flags
    unsigned int* d_dupbits = nullptr; size_t d_dupbits_cap = 0; // [K][buckets][words] duplicate bitmaps
    // bucketed plan (kernels_plan.hip): references per (step, row range), scatter cursors, bucket lists
    int* d_pl_cnt = nullptr;   size_t d_pl_cnt_cap = 0;          // [K][3 ranges + 1]: counts, cursors, offsets
    const void* pl_cnt_clean = nullptr; size_t pl_cnt_clean_cap = 0; int pl_cnt_nb = -1;      // the buffer (and ranges per step) whose counts and cursors are all zero between plans
    int2* d_pl_list = nullptr; size_t d_pl_list_cap = 0;         // [K][references per step] (id, output position | role << 30)
    bool plan_big = false;                                       // the last plan met a bucket of > 16 k references: 1024-thread workgroups
    int pair_gen = 0; const void* partner_zeroed = nullptr; size_t partner_zeroed_cap = 0;      // generation of the last pairing plan; the partner buffer (pointer, size) that has been zeroed
    int pair_pause = 0;                                          // pairing: calls left before it is tried again (the last plan that paired accepted too few rows to pay for itself)
    // pairing (kernels_plan.hip, "pairing"): the two references of a row referenced exactly twice are brought into one wavefront
    int4* d_partner = nullptr; size_t d_partner_cap = 0;         // [K][B] per triplet: where the partner of its slot 0 / 1 / 2 sits if that row is referenced exactly twice (generation-tagged words, ORX_PARTNER_*)
    int* d_pslot = nullptr;    size_t d_pslot_cap = 0;           // [K][2B] parallel to dlist: position of the FIRST reference of a row referenced exactly twice (-1: another kind of row)
    int4* d_ids4 = nullptr;    size_t d_ids4_cap = 0;            // [K][B] the fused kernel's input with pairing, written by the plan itself: (user, pos, neg) rewritten ids of position j, pairing word | origin << 10
    const float* plan_label = nullptr;                           // pointwise step with pairing: the labels of the chunk being planned (DedupArgs::label)
    int* h_plan = nullptr;                                       // pinned host mirror of the per-step plan counters
    size_t h_plan_cap = 0;
    hipEvent_t plan_ev = nullptr;                                // "plan counters have arrived on the host"
    // What the counters of the LAST plan that was looked at said (api.hip, "no read-back"): a pairwise call whose predecessor was quiet
    // -- no range wanted a staging plan, few duplicated rows, no oversized bucket -- makes its plan with staging off, launches every step
    // without waiting for its own counters and leaves them for the next call to look at (stats_ev: their copy has arrived).
    struct { bool valid = false, quiet = false; int64_t key[5] = {0, 0, 0, 0, 0}; } plan_stats;
    int64_t stat_pairs = 0, stat_max_dup = 0, stat_nowait_calls = 0;      // orx_ctx_stat
    hipEvent_t stats_ev = nullptr;
    bool stats_pending = false; int64_t stats_kc = 0, stats_B = 0; bool stats_pairing = false; int stats_age = 0; int64_t stats_key[5] = {0, 0, 0, 0, 0};
    hipEvent_t wait_ev = nullptr;                                // orx_ctx_wait_stream
    int epoch = 0;                                               // step epoch: tags ready flags and censor side marks
    int epoch_gen = 0;                                           // bumped when `epoch` wraps (tables then clear their tags)
    // staging plan of rows referenced >= 3 times in a step (see kernels_pairwise.hip, "staging")
    int2* d_refinfo = nullptr; size_t d_refinfo_cap = 0;         // [K][3Bp] (dense row, rank) of role-2 references
    int* d_tricnt = nullptr;   size_t d_tricnt_cap = 0;          // [K][B] references per dense row
    int* d_segstart = nullptr; size_t d_segstart_cap = 0;        // [K][B] first staging slot per dense row
    int* d_alloc = nullptr;    size_t d_alloc_cap = 0;           // [K][8] allocators: dense rows, staging slots, tree items per level
    int* d_dseg = nullptr;     size_t d_dseg_cap = 0;            // [K][2B] parallel to dlist: staging segment start
    int* d_dcnt = nullptr;     size_t d_dcnt_cap = 0;            // [K][2B] parallel to dlist: segment length (0: two-reference row, <0: long)
    int4* d_chunks = nullptr;  size_t d_chunks_cap = 0;          // [K][item_stride] work items of the reduction tree over long segments
    float* d_part = nullptr;   size_t d_part_cap = 0;            // [item_stride][D] partial sums of the tree (one step at a time)
    float* d_partb = nullptr;  size_t d_partb_cap = 0;           // [item_stride] the same for the bias gradients
    float* d_stage = nullptr;  size_t d_stage_cap = 0;           // [2][3B][D] staged gradients (double-buffered by step parity)
    float* d_stageb = nullptr; size_t d_stageb_cap = 0;          // [2][3B] staged bias gradients
    uint32_t* d_dlist = nullptr; size_t d_dlist_cap = 0;         // [K][2B] duplicated rows
    int* d_dcount = nullptr;   size_t d_dcount_cap = 0;          // [K]
    float* d_partial = nullptr; size_t d_partial_cap = 0;   // [K][nwaves][2] loss partials
    double* d_loss = nullptr;  size_t d_loss_cap = 0;       // [K][2] step results
    float* d_tmp = nullptr;    size_t d_tmp_cap = 0;        // misc fp32 scratch
    unsigned char* d_topk = nullptr; size_t d_topk_cap = 0;  // top-K: thresholds, candidate lists, exclusion rows, staged outputs
    float* d_wpart = nullptr;  size_t d_wpart_cap = 0;      // [nwaves][D] dense-kernel gradient partials
    // deterministic row apply (kernels_rowsort.hip): ping-pong buffers of the radix sort, its histograms, partial sums of runs
    // that cross a 64-entry block
    uint2* d_sort[2] = {nullptr, nullptr}; size_t d_sort_cap[2] = {0, 0};
    int* d_sort_hist = nullptr; size_t d_sort_hist_cap = 0;
    float* d_csr_part[2] = {nullptr, nullptr}; size_t d_csr_part_cap[2] = {0, 0};
    float* d_splitk = nullptr; size_t d_splitk_cap = 0;     // [splits][M][N] partial products of a split-K fp32 product
    bool prof = false;
    ProfSlot prof_slot[ORX_K_NUM];
    std::vector<int> prof_order;                     // kernel class of every profiled launch, in launch order (ORX_PROF_TIMELINE)
    hipEvent_t cur_e0 = nullptr, cur_e1 = nullptr;   // events of the launch being profiled (or null)
    int num_cu = 256;
};

struct orx_table {
    orx_ctx* ctx = nullptr;
    float* w = nullptr;               // [rows, dim]
    int64_t rows = 0;
    int32_t dim = 0;
    bool owned = true;
    // per-step scratch, allocated on first use by a train step
    float* gsum = nullptr;            // [rows, dim] duplicate-row gradient sums (all-zero between steps)
    float* gsum2 = nullptr;           // second scratch rows of the pairwise step (rows referenced exactly twice)
    int* ready = nullptr;             // [rows] ready flags of the in-launch duplicate apply
    int tag_gen = 0;                  // ctx->epoch_gen the ready / side tags belong to
    int* side = nullptr;              // [rows][2] fused censor: last epoch with a duplicated pos / neg reference
    struct orx_opt* lazy = nullptr;   // lazily-applied Adam: rows are caught up on demand (orx_table_sync flushes)
    uint64_t version = 0;             // bumped by every host-side write / fill / init and by the dense optimizer kernels: derived copies
                                      // (the fp16 copies of the DLRM kernels) know when they are stale
};

struct OptSlots {
    float* s0 = nullptr;              // Adagrad acc / Adam m / momentum velocity
    float* s1 = nullptr;              // Adam v
    int* last = nullptr;              // lazy Adam: optimizer step up to which (w, m, v) of the row are current
};

struct orx_opt {
    orx_ctx* ctx = nullptr;
    int kind = ORX_SGD;
    float lr = 0.01f, p0 = 0.f, p1 = 0.f, p2 = 0.f;
    int64_t t = 0;                    // Adam step counter
    std::map<orx_table*, OptSlots> slots;
    // lazy Adam: lr_t of every step taken so far (index = step), host mirror + device copy
    std::vector<float> h_lrt; float* d_lrt = nullptr; size_t lrt_cap = 0; int64_t lrt_uploaded = 0;
    // closed-form replay (round 6, orx_device.h adam_cf_*): per step k the three moments V_q[k] = sum_{j=1..J} b1^j j^q lr_{k+j}, q = 0, 1, 2
    // (float4 per step, w unused); entries [0, lrv_done) are final for the present learning rate
    std::vector<float> h_lrv; float* d_lrv = nullptr; size_t lrv_cap = 0; int64_t lrv_done = 0;
};
// the second scalar of the sum-then-apply rules (the kernels' `eps` argument): Adagrad's epsilon; for momentum the
// momentum, its sign bit set for nesterov (orx_device.h mom_elem; -0.0f for nesterov with momentum 0)
inline float orx_rule_eps(const orx_opt* o) {
    if (o->kind == ORX_ADAGRAD) return o->p1;
    if (o->kind == ORX_MOMENTUM) return o->p1 != 0.f ? -o->p0 : o->p0;
    return 0.f;
}
constexpr int ORX_ADAM_CF_TERMS = 512;        // J: b1^J is negligible for b1 <= 0.95
// what a kernel needs for the closed-form replay: the moments table and the constants (lrv NULL: the replay loops)
struct AdamCFParams { const float4* lrv; float delta, lb1, lb2; };
AdamCFParams orx_adam_cf_params(const orx_opt* o);
bool orx_adam_cf_ok(const orx_opt* o);        // closed-form replay applicable (b1 <= 0.95, 1 - sqrt(b2) <= 1e-3)
// Lazily-applied TF-2.0 Adam: the dense decay of a row that no triplet touches (m *= b1, v *= b2, w -= lr_t m /
// (sqrt(v)+eps), every step) is replayed exactly when the row is next needed.  orx_table_sync brings every row of a
// table up to the optimizer's current step; every entry point that reads or writes a table calls it first.
int orx_table_sync(orx_table* t);
int orx_opt_isolate(orx_opt* o, orx_table* const* keep, int n_keep);   // finish every OTHER table that is lazy under `o`
int orx_opt_last(orx_opt* o, orx_table* t, bool restamp, int** out, int64_t stamp = -1);            // allocate / fetch the per-row step stamps
int orx_launch_fill_int(orx_ctx* ctx, int* p, int64_t n, int v);
int orx_adam_lrt(orx_opt* o, int64_t upto);                      // make lr_t of steps 1..upto available on the device
int orx_launch_adam_flush(orx_ctx* ctx, float* w, float* m, float* v, int* last, int64_t rows, int dim, int t_end, const float* lrt,
                          float b1, float b2, float eps, struct AdamCFParams cf);

// ------------------------------------------------------- helpers (api.hip) ---
int orx_ensure(void** p, size_t* cap, size_t bytes);           // grow a device buffer
int orx_table_scratch(orx_table* t, bool second = false);       // allocate gsum (and gsum2)
int orx_table_side(orx_table* t);                               // allocate the fused-censor side marks
int orx_opt_slots(orx_opt* opt, orx_table* t, OptSlots* out);   // allocate optimizer slots
int stage_ids(orx_ctx* c, const int32_t* host, int64_t n, int64_t off);   // H2D into ctx->d_ids
int fetch_losses(orx_ctx* c, int64_t K, float* loss_out, float* l2_out);

// ---------------------------------- the host driver of the train steps (api_steps.hip) ---
struct Carve {                                // consecutive 256-byte aligned pieces of one device buffer
    size_t off = 0;
    size_t take(size_t bytes) { const size_t at = off; off += (bytes + 255) & ~(size_t)255; return at; }
};
// One input list of a K-step call, `width` 4-byte elements per sample (p NULL: the call has no such list), and where the lists
// are once staged: the elements of step s of a list begin at its pointer + s * ds * width.
struct StepList { const void* p; int width; };
struct StepInputs { const int32_t* id[3]; const float* f[2]; int64_t ds; };
// Device lists (ORX_IDS_DEVICE) pass through with ds = id_stride; host lists are packed at B * width elements per step, the ids
// into ctx->d_ids and the floats into ctx->d_lab (one copy per list where the host array is packed already), with ds = B.
int orx_stage_steps(orx_ctx* c, int64_t K, int64_t B, int64_t id_stride, int flags, std::initializer_list<StepList> ids,
                    std::initializer_list<StepList> floats, StepInputs* in);
constexpr int64_t ORX_STEP_CHUNK = 32;        // steps whose loss partials one loss_reduce launch sums (and whose id lists the subset route sorts together)
// K steps in chunks of min(K, ORX_STEP_CHUNK): chunk(s0, kc) before a chunk's steps (empty: nothing), step(s, i, partial) for step
// s = s0 + i with the np (loss, l2) partials it writes, one loss_reduce per chunk when a loss is wanted; then the losses are
// fetched and, for host ids, the index flag is looked at.  d_partial and d_loss are sized here, before the first pointer into them.
int orx_run_steps(orx_ctx* c, int64_t K, int np, int flags, float* loss_out, float* l2_out,
                  const std::function<int(int64_t, int64_t)>& chunk, const std::function<int(int64_t, int64_t, float*)>& step);
// a forward-only entry point: forward(partial) launches one step's forward; its np partials are summed and fetched, the index flag
// is looked at wherever the ids live
int orx_run_forward(orx_ctx* c, int np, float* loss_out, float* l2_out, const std::function<int(float*)>& forward);
// The checks every family that scores by dot products over (U, V, b) makes, with `fn` in front of each message.  The model
// (step and forward alike): NULLs, contexts, U->dim == V->dim + extra_dim (VBPR: the projection width), the bias shape, flags outside `allowed`, ORX_HOGWILD / ORX_CENSOR.
// The step: the model's, then the optimizer, l2_reg, ORX_NO_L2, K / B / id_stride, what orx_apply_rows would refuse, the counter.
int orx_check_dot_model(const char* fn, orx_ctx* c, orx_table* U, orx_table* V, orx_table* b, int extra_dim, int flags, int allowed);
int orx_check_dot_step(const char* fn, orx_ctx* c, orx_opt* opt, orx_table* U, orx_table* V, orx_table* b, int extra_dim,
                       int64_t K, int64_t B, int64_t id_stride, float l2_reg, int flags, int allowed);
int orx_check_apply_rows_opt(const orx_opt* opt, const orx_table* t, const orx_table* bias);      // orx_apply_rows' refusal of an optimizer kind, with its message
// lazy tables: the rows a step reads are replayed to the optimizer's step (no-ops for a table that is current) -- U with the user
// list, V and b with each item list (i1 NULL: one list)
int orx_touch_step(orx_table* U, orx_table* V, orx_table* b, const int32_t* uid, int64_t nu, const int32_t* i0, int64_t n0,
                   const int32_t* i1, int64_t n1);
// orx_rows_sort of K lists with the pairs left in `keep` ([K][n], the caller's): the sort's own output lasts until the context's next sort
int orx_rows_sort_keep(orx_ctx* c, const int32_t* ids, int64_t K, int64_t n, int64_t id_stride, int64_t rows, uint2* keep);
// orx_apply_rows' deterministic route on a list that is sorted already: the table is synced unless it is lazy under `opt`
int orx_apply_rows_sorted(orx_ctx* c, orx_opt* opt, orx_table* t, const uint2* sorted, int64_t n, const float* grads, int64_t g_stride);
// ---------------------------------- the host driver of the scoring, top-K and ranking-metric calls (api_eval.hip) ---
constexpr int ORX_EVAL_NAT = 16;              // most cut-offs of one metrics call (the kernels keep them in a fixed array)
int orx_sync_tables(std::initializer_list<orx_table*> tables);        // orx_table_sync of each (NULL entries skipped): first, before the argument checks
// The scorer's argument checks (U and V not NULL), `fn` in front of each message: kind, U->dim == V->dim and the bias [items, 1], GMF's
// w [D, 1], dim <= 1024 -- ORX_ERR_ARG -- and, for the calls that check their host user ids before any device work, ORX_ERR_INDEX
int orx_check_scorer(const char* fn, orx_ctx* c, int kind, orx_table* U, orx_table* V, orx_table* b, orx_table* w,
                     const int32_t* uid, int64_t n, bool check_uid_on_host);
// CSR lists over n users (ptr not NULL): offsets from 0 that never decrease, ids inside [0, NI) (ORX_ERR_INDEX, naming the user),
// with `ascending` every row strictly ascending; *longest (may be NULL): the longest row
int orx_check_lists(const char* fn, const char* what, const int64_t* ptr, const int32_t* items, int64_t n, int64_t NI,
                    bool ascending, int64_t* longest);
// The lists of users [q0, q0 + nq) of a CSR, offsets rebased to 0 (hp [nq + 1], the caller's, alive until the stream is synchronised):
// one async copy per piece on c->stream (sorted not NULL: the item slice goes through it, sorted inside each row), or offsets and item
// slice written into a caller's packed host buffer
struct CsrSlice { int64_t first, count, longest; };   // items [first, first + count) of the CSR; the batch's longest row
int orx_stage_csr(orx_ctx* c, const int64_t* ptr, const int32_t* items, int64_t q0, int64_t nq, int64_t* hp,
                  std::vector<int32_t>* sorted, int64_t* d_ptr, int32_t* d_items, CsrSlice* out);
CsrSlice orx_pack_csr(const int64_t* ptr, const int32_t* items, int64_t q0, int64_t nq, int64_t* hp, void* hi);
size_t orx_layout(const size_t* sizes, int n, size_t* off);           // consecutive 256-byte aligned pieces: their offsets, the total
int64_t orx_largest_batch(int64_t lo, int64_t hi, const std::function<bool(int64_t)>& fits);     // the largest m in [lo, hi] that fits (fits monotone; lo if none does)
// Score rows of a batch of nq users in a call of n users on the dense route.  A call of more than 64 users scores at least 65 rows
// in every launch: the scorer's tile holds 128 users then, and its L2 norms are only bit-stable within one tile shape
// (kernels_topk.hip) -- so a short last batch computes what the one-batch call computes.
inline int64_t orx_dense_rows(int64_t n, int64_t nq) { return n > 64 && nq < 65 ? 65 : nq; }
int orx_stage_uid_rows(orx_ctx* c, const int32_t* uid, int64_t nq, int64_t rows);     // nq host ids into d_ids (grown here), padded to `rows` with the first
int orx_evalbits_reserve(orx_ctx* c, size_t bytes);                   // grow d_evalbits; a new buffer starts out all zero
// buckets of the rank kernels: 2^STEPS, STEPS from the call's longest positive list as rank_sweep_kernel picks it
inline int orx_rank_buckets(int64_t max_pos) { return max_pos <= 7 ? 8 : (max_pos <= 15 ? 16 : 64); }
// async copies of the metrics of users [q0, q0 + nq) to the host outputs that are not NULL
int orx_fetch_metrics(orx_ctx* c, const float* d_auc, const float* d_ndcg, const float* d_rec, int64_t q0, int64_t nq, int nat,
                      float* auc, float* ndcg, float* recall);
// One batch of the CSR metrics over users [q0, q0 + nq) of a call of n users: one packed upload (the lists rebased, the cut-offs), the
// bitmaps, the scores (host pred, device pred, or the scorer over orx_dense_rows rows when pred is NULL), the sweeps, one packed
// download; outputs land at row q0.  Leaves the bitmaps all zero whether it succeeds or not.
struct RankCsrCall {
    const char* fn; int kind; orx_table* U; orx_table* V; orx_table* b; orx_table* w; const int32_t* uid;
    const float* pred; bool pred_on_device;               // [n, items], NULL: the scorer
    int64_t n, items;
    const int64_t* pos_ptr; const int32_t* pos_items; const int64_t* excl_ptr; const int32_t* excl_items;
    const float* at; int nat; int64_t max_pos;            // max_pos: the CALL's longest positive list (every batch takes the call's chunking)
    float* auc; float* ndcg; float* recall;
};
int orx_rank_csr_run(orx_ctx* c, const RankCsrCall& k, int64_t q0, int64_t nq);
// the bodies of the train steps with the objective's two knobs exposed (api_weighted.hip): per-triplet weights (NULL: all ones) and
// the coefficient l2w of l2_loss; the plain entry points pass NULL and 0 / 1
int orx_pairwise_step_impl(orx_ctx* c, int model, orx_opt* opt, orx_table* U, orx_table* V, orx_table* b,
                           const int32_t* uid, const int32_t* pid, const int32_t* nid, const float* weight,
                           int64_t K, int64_t B, int64_t id_stride, float margin, float l2w, int flags, float* loss_out, float* l2_out);
int orx_pairwise_loss_impl(orx_ctx* c, int model, orx_table* U, orx_table* V, orx_table* b,
                           const int32_t* uid, const int32_t* pid, const int32_t* nid, const float* weight,
                           int64_t B, float margin, int flags, float* loss_out, float* l2_out);
int orx_pairwise_subset_impl(orx_ctx* c, int model, orx_opt* opt, orx_table* U, orx_table* V, orx_table* b,
                             const int32_t* uid, const int32_t* pid, const int32_t* nid, const float* weight,
                             int64_t K, int64_t B, int64_t id_stride, float margin, float l2w, int flags, int train_mask,
                             float* loss_out, float* l2_out);
int orx_pointwise_step_impl(orx_ctx* c, int model, orx_opt* opt, orx_table* U, orx_table* V, orx_table* b, orx_table* w,
                            const int32_t* uid, const int32_t* iid, const float* label,
                            int64_t K, int64_t B, int64_t id_stride, float a_w, float b_w, float l2w, int flags, float* loss_out, float* l2_out);
int orx_pointwise_subset_impl(orx_ctx* c, int model, orx_opt* opt, orx_table* U, orx_table* V, orx_table* b, orx_table* w,
                              const int32_t* uid, const int32_t* iid, const float* label,
                              int64_t K, int64_t B, int64_t id_stride, float a_w, float b_w, float l2w, int flags, int train_mask,
                              float* loss_out, float* l2_out);
// host setup the pairwise and the pointwise step call share (api.hip)
int orx_fallback_bits();                                          // ORX_FORCE_FALLBACK, read per call
int orx_epochs_reserve(orx_ctx* c, int64_t K, std::initializer_list<orx_table*> tables);     // K step epochs; on wrap-around the tables clear their tags
int orx_apply_blocks(int64_t B, int D);                           // blocks of a step's launch that apply the previous step's duplicated rows
int orx_adam_dense_step(orx_ctx* c, orx_opt* opt, std::initializer_list<std::pair<orx_table*, OptSlots>> tables, float* lr_t_out);
// lazy Adam, what PairArgs and PointArgs share: second slots, per-row step stamps (restamp: the tables were not lazy under
// `opt` so far), lr_t of the K steps to come, the constants of the replay; the tables become lazy under `opt`.  b may be NULL.
template <class Args>
int orx_lazy_adam_fill(orx_opt* opt, orx_table* U, orx_table* V, orx_table* b, const OptSlots& sU, const OptSlots& sV, const OptSlots& sb,
                       bool restamp, int64_t K, Args* a) {
    a->a2U = sU.s1; a->a2V = sV.s1; a->a2b = sb.s1;
    CHECK(orx_opt_last(opt, U, restamp, &a->lastU)); CHECK(orx_opt_last(opt, V, restamp, &a->lastV));
    if (b) CHECK(orx_opt_last(opt, b, restamp, &a->lastb));
    CHECK(orx_adam_lrt(opt, opt->t + K));
    a->lrt = opt->d_lrt; a->b1 = opt->p0; a->b2 = opt->p1; a->eps = opt->p2;
    const AdamCFParams cf = orx_adam_cf_params(opt);              // (lrv NULL: the replay loops)
    a->lrv = cf.lrv; a->cf_delta = cf.delta; a->cf_lb1 = cf.lb1; a->cf_lb2 = cf.lb2;
    a->newton = (1.0f - sqrtf(opt->p1)) <= 1e-3f;
    U->lazy = opt; V->lazy = opt;
    if (b) b->lazy = opt;
    return ORX_OK;
}
void orx_prof_begin(orx_ctx* ctx, int kid);
void orx_prof_end(orx_ctx* ctx, int kid);

// While a ProfScope is alive, ORX_LAUNCH attaches a (start, stop) event pair to
// the kernel dispatch itself (hipExtLaunchKernelGGL), i.e. the events carry the
// kernel's own begin/end timestamps -- the same quantity rocprofv3 reports.
struct ProfScope {
    orx_ctx* c; int k;
    ProfScope(orx_ctx* c_, int k_) : c(c_), k(k_) { if (c->prof) orx_prof_begin(c, k); }
    ~ProfScope() { if (c->prof) orx_prof_end(c, k); }
};

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per device: one bit per device ordinal, per call site
#define ORX_ONCE_PER_DEVICE(ctx, stmt)                                                  \
    do {                                                                               \
        static unsigned long long _done = 0ull;                                        \
        const unsigned long long _bit = 1ull << ((ctx)->device & 63);                  \
        if (!(_done & _bit)) { stmt; _done |= _bit; }                                  \
    } while (0)

#define ORX_LAUNCH(ctx, kernel, grid, block, shm, ...)                                 \
    hipExtLaunchKernelGGL(kernel, grid, block, shm, (ctx)->stream, (ctx)->cur_e0, (ctx)->cur_e1, 0, __VA_ARGS__)

// ------------------------------------------------ kernel launch parameters ---
// Duplicate detection output, per step (reference index r: user lookup k -> k,
// pos-item lookup k -> B + k, neg-item lookup k -> 2B + k):
//   ids_out[r] = id | (dup << 31): the id with "row referenced more than once in this batch" in bit 31
//                (the pairwise fused kernel reads these instead of the caller's ids); dflag[r] = the same
//                flag as a byte (pointwise / censor / apply_rows)
//   dlist[...] = the distinct duplicated rows of the step: row | (is_item << 31)
//   dcount     = number of entries in dlist
struct PairArgs {
    float* U; float* V; float* b;
    float* gU; float* gV; float* gb;          // duplicate-row gradient sums (zero between steps)
    float* gU2; float* gV2; float* gb2;       // second scratch rows (rows referenced exactly twice), may be NULL
    float* aU; float* aV; float* ab;          // Adagrad accumulators / Adam m
    float* a2U; float* a2V; float* a2b;       // Adam v
    int* lastU; int* lastV; int* lastb;       // lazy Adam: per-row step stamps (NULL: not the lazy Adam path)
    const float* lrt; float b1; float b2; int step_t;   // lr_t per step, betas, index of THIS step (its lr_t = lrt[step_t])
    int newton;                 // lazy Adam: carry 1/(sqrt(v)+eps) by Newton steps (1 - sqrt(beta_2) <= 1e-3)
    int long_gap;               // lazy Adam: tables large relative to the batch (rows wait hundreds of steps): LONGGAP kernel
    const float4* lrv;          // lazy Adam, closed-form replay: V_q per step (orx_opt::d_lrv), NULL: the replay loops
    float cf_delta, cf_lb1, cf_lb2;     // -ln sqrt(b2), log2 b1, log2 b2
    const int32_t* uid; const int32_t* pid; const int32_t* nid;
    const int4* ids4;                         // pairing: [B] (user, pos item, neg item) rewritten ids of the triplet processed at position j and, in w, its pairing
                                              // word (ORX_PAIR_*, bits 9:0) and the triplet's original position (bits 31:10); NULL: uid / pid / nid as usual
    int role_bits;                            // ids carry role (bits 30:29) and urgent (bit 28): tables < 2^28 rows
    // in-launch application of the PREVIOUS step's duplicated rows (n_apply_blocks == 0: off)
    int n_apply_blocks; int epoch;
    const uint32_t* prev_dlist; const int* prev_dcount;
    int censor; float min_norm;               // censor_vec fused into the row write-back (fast dims, exact mode)
    int* sideV;                               // [NI][2] epoch of the last step that referenced the item as a duplicated pos / neg
    int* readyU; int* readyV;                 // per-row ready flags (value = epoch of the launch that applied the row)
    const uint32_t* dlist;                    // duplicated rows of this step
    const int* dcount;
    // staging of rows referenced >= 3 times (NULL stage: such references use atomics into gsum)
    const int2* refinfo; const int* segstart;         // this step
    float* stage; float* stageb;                      // this step's staging buffers
    const int* dseg; const int* dcnt;                 // parallel to dlist
    const float* prev_stage; const float* prev_stageb; const int* prev_dseg; const int* prev_dcnt;   // step s-1 (in-launch apply)
    const int4* items; const int* nitems;             // reduction tree over this step's long segments (hot_reduce_kernel):
    float* part; float* partb;                        //   items of level l at items + tree_off[l], count nitems[l]; partial sums
    int tree_off[3];
    int64_t B; int64_t NU; int64_t NI;
    int D;
    float lr; float eps; float margin; float invB; float l2w;
    float* partial;                           // [nwaves][2] loss / l2 partials of this step
    int no_loss;                              // the caller takes neither the loss nor the l2 sum: kernels with a loss-free form skip the partials (fused_kernel LOSS)
    int* err;
    const float* wt;                          // [B] this step's per-triplet weights in the CALLER's order (orx_pairwise_step_weighted), NULL: all ones
};

struct DedupArgs {
    const int32_t* uid; const int32_t* pid; const int32_t* nid;   // step 0 of the chunk
    int64_t id_stride;                        // elements between consecutive steps
    unsigned char* dflag;                     // [K][flag_stride] or NULL
    int32_t* ids_out;                         // [K][flag_stride] or NULL: id | (dup << 31); 0x7fffffff = invalid id
    unsigned int* dupbits;                    // [K][nbu+nbi][DD_WORDS] "seen twice" bitmaps kept for urgent_kernel, or NULL
    unsigned char* roles;                     // [K][flag_stride] scratch (pass 1 -> pass 2) or NULL: no role bits
    int64_t role_stride;                      // ids_out layout [3][role_stride] per step (0: compact reference order)
    uint32_t* dlist;                          // [K][list_stride]
    int* dcount;                              // [K], zeroed before the launch
    int64_t flag_stride; int64_t list_stride;
    // reference numbering: user refs [0, nU), then pid refs [nU, nU+nP), then nid refs [nU+nP, nU+nP+nN)
    int64_t nU; int64_t nP; int64_t nN;
    int64_t NU; int64_t NI;                   // table rows
    int nbu; int nbi;                         // row-range buckets per table (0 = table not scanned)
    int first_only;                           // censor: dflag = 1 only on non-first references
    // column windows (DLRM): the item id stream is an [nP / col_F][col_F] matrix whose column c only holds rows of one
    // table; item range bk scans columns col_win[bk].x .. +col_win[bk].y-1 only (NULL: the whole stream)
    int col_F; const int2* col_win;
    // staging plan (all NULL: rows referenced >= 3 times keep role 2 = atomics)
    int2* refinfo;                            // [K][flag_stride]
    int* tricnt; int* segstart;               // [K][tri_stride], tricnt zeroed before the launch
    int* alloc;                               // [K][8], zeroed before the launch: 0 dense rows, 1 staging slots, 2.. tree items of level 1, 2, 3
    int* dseg; int* dcnt;                     // [K][list_stride]
    int4* items;                              // [K][item_stride] tree work items (src, len, dst, -), level l at offset tree_off[l]
    int64_t tri_stride; int64_t item_stride;
    int tree_off[3];
    int min_late;                             // bucketed plan: see PairPlan
    // pairing (bucketed plan only; pair_tpw < 2: off): triplets per wavefront of the fused kernel that will run the steps,
    // per-step arrays [K][pair_stride] partner (16-byte record per triplet) and ids4, [K][2 list_stride] pslot; the number of accepted pairs
    // of step s is alloc[8 s + 7]
    int pair_tpw; int4* partner; int* pslot; int4* ids4; int64_t pair_stride;
    int pair_gen;                             // generation tag (1 .. 63) of this plan's partner words: see ORX_PARTNER_* below
    // pointwise steps (two id lists, nN = 0) with pairing: word z of a sample's input record carries its LABEL (the bits of the float)
    // instead of a third id -- it travels with the ids when plan_swap_kernel moves the sample.  [K][id_stride], NULL: pairwise
    const float* label;
};
// pairing word of a triplet (PairArgs::pinfo): the triplet shares one row with the triplet of lane group PARTNER of the same wavefront;
// the WRITER adds the partner's gradient of that row to its own and updates the row in place, the other one does not write it
// A word of a triplet's pairing record partner[t].{x,y,z}: bits 23:0 the position of the other reference of that slot's row, bit 30
// "this is the row's second reference", bits 29:24 the GENERATION of the plan that wrote it.  The records are never initialised per
// plan (16 bytes per triplet and step, a fifth of what plan_part_kernel<true> wrote): a word counts only if it carries the current
// plan's generation; the buffer is zeroed when it is allocated and whenever the generations wrap (every 63 plans).  Position
// ORX_PARTNER_POISON marks a triplet with an out-of-range id (written for such triplets only): never paired.
constexpr uint32_t ORX_PARTNER_POS = 0x00ffffffu, ORX_PARTNER_POISON = 0x00ffffffu;
constexpr uint32_t ORX_DLIST_DEAD = 0xffffffffu;     // entry of a step's list of duplicated rows whose row was paired after all: nothing to apply
constexpr uint32_t ORX_PAIR_VALID = 0x200u, ORX_PAIR_WRITER = 0x100u;      // bits 3:0 partner lane group, 5:4 my slot (0 user, 1 pos, 2 neg), 7:6 partner's slot
constexpr int ORX_SEG_DIRECT = 16;            // the apply sums up to this many staged gradients / partial sums of a row itself
constexpr int ORX_PIECE = 64;                 // longer segments: a tree of 64-to-1 partial sums (hot_reduce_kernel, one wavefront per piece)

struct ReduceArgs {
    const float* partial;                     // [K][nwaves][2]
    double* out;                              // [K][2]
    int nwaves;
};

struct RowsArgs {                              // sharded building blocks (kernels_sharded.hip)
    float* W; float* bias;                    // table [rows, D], bias [rows] or NULL
    float* G; float* gb;                      // gsum scratch
    float* A; float* ab;                      // Adagrad accumulators
    const int32_t* ids;                       // local row ids, < 0 = skip
    const unsigned char* dflag;
    const float* grads; int64_t g_stride;     // [n, g_stride]; bias gradient at column D ...
    const float* gbias;                       // ... or, if not NULL, in this array [n] (apply_rows_sgd_flagged_kernel)
    int64_t n; int64_t rows; int D;
    float lr; float eps;
    int* err;
    // planned apply (orx_apply_rows_planned): ids rewritten by dedup_kernel (item role), scratch rows, staging
    const int32_t* ids2; float* G2; float* gb2;
    const int2* refinfo; const int* segstart; float* stage; float* stageb;
};

struct AdamRowsArgs {                          // lazy TF-2.0 Adam on gradient rows (kernels_sharded.hip)
    float* W; float* M; float* V; int* last;  // table, slots, per-row step stamps
    float* G;                                 // gsum scratch (duplicated rows)
    const int32_t* ids;                       // local row ids, < 0 = skip
    const unsigned char* dflag; const uint32_t* dlist; const int* dcount;    // dedup of ids (item role)
    const float* grads; int64_t g_stride;
    int64_t n; int64_t rows; int D;
    const float* lrt; float lr_T; float b1; float b2; float eps;
    int T; int newton;
    int* err;
    AdamCFParams cf;                          // closed-form replay (orx_device.h AdamCF)
};
int orx_launch_adam_rows(orx_ctx* ctx, bool step, const AdamRowsArgs& a, int64_t max_dups);
// lazy Adam on a table's gradient rows: replay the rows of `ids` to the optimizer's step (touch) / take step opt->t
struct ColWindows { int F = 0; const int2* win = nullptr; };    // device array, one entry per 425 984-row range of the table
int orx_adam_rows_dedup(orx_ctx* ctx, orx_table* t, const int32_t* ids, int64_t n, ColWindows cw = ColWindows());
int orx_adam_rows_touch(orx_ctx* ctx, orx_opt* opt, orx_table* t, const int32_t* ids, int64_t n, bool have_dedup, ColWindows cw = ColWindows());
int orx_adam_rows_apply(orx_ctx* ctx, orx_opt* opt, orx_table* t, const int32_t* ids, int64_t n, const float* grads, int64_t g_stride,
                        bool have_dedup, ColWindows cw = ColWindows());
int orx_summed_rows_apply(orx_ctx* ctx, orx_opt* opt, orx_table* t, orx_table* bias, const int32_t* ids, int64_t n, const float* grads,
                           int64_t g_stride, ColWindows cw = ColWindows());
int orx_table_touch(orx_table* t, const int32_t* ids, int64_t n);       // no-op unless the table is lazy
bool orx_adam_rows_lazy(const orx_opt* opt, const orx_table* t);

struct GradArgs {
    const float* u; const float* p; const float* n; int64_t row_stride;   // gathered rows, bias at column D
    const int32_t* valid;                     // triplet k is live iff valid == NULL or valid[k] >= 0
    float* gu; float* gp; float* gn; int64_t g_stride;
    int64_t T; int D;
    float invB; float margin; float l2w;
    float* partial;
};

int orx_launch_pair_grads(orx_ctx* ctx, int model, const GradArgs& a, int* nwaves);
int orx_launch_apply_rows(orx_ctx* ctx, int optkind, bool use_dflag, const RowsArgs& a);
bool orx_launch_apply_rows_pair(orx_ctx* ctx, const RowsArgs& a, const RowsArgs& b, int* rc);
int orx_launch_loss_accumulate(orx_ctx* ctx, const float* partial, int64_t nwaves, double* accum);
int orx_shard_grads_nwaves(int D, int64_t T);

// partial train step (kernels_subset.hip, api_subset.hip): one gradient launch per step; an output pointer that is NULL names a
// role the step does not train -- nothing is written for it
struct SubsetArgs {
    const float* U; const float* V; const float* b;               // read only (b NULL: BPR without item biases)
    const int32_t* uid; const int32_t* pid; const int32_t* nid;   // this step's ids (WRMF: pid = item ids, nid unused)
    const float* label;                                           // WRMF
    float* gu; float* gi; float* gb;                              // [B][D]; [2B][D] and [2B]: positive lookups, then negative (WRMF: [B][D], [B])
    int64_t B; int64_t NU; int64_t NI;
    int D;
    float invB; float margin; float l2w; float a_w; float b_w;
    int sigmoid;
    float* partial;                                               // [orx_fused_nwaves(D, B)][2] loss / l2 partials of this step
    int* err;
    const float* wt;                                              // [B] per-triplet weights of this step (pairwise), NULL: all ones
};
int orx_launch_subset_grads(orx_ctx* ctx, int model /* ORX_BPR, ORX_UCML, MODEL_BPR_NB; < 0: WRMF */, const SubsetArgs& a);
int orx_launch_subset_concat_ids(orx_ctx* ctx, const int32_t* pid, const int32_t* nid, int64_t id_stride, int64_t K, int64_t B, int32_t* out);

// pointwise (GMF / WRMF) step, kernels_pointwise.hip
struct PointArgs {
    float* U; float* V; float* b; const float* w;
    float* gU; float* gV; float* gb;
    float* aU; float* aV; float* ab;
    const int32_t* uid; const int32_t* iid; const float* label;
    const unsigned char* dflag;               // [2B]: user refs then item refs (tables >= 2^28 rows / generic dims)
    // exact mode with role bits: uid / iid are the ids REWRITTEN by dedup_kernel (flag 31, role 30:29), iid = uid + Bp
    int role_bits;
    float* gU2; float* gV2; float* gb2;       // second scratch rows (rows referenced exactly twice)
    const int2* refinfo; const int* segstart; float* stage; float* stageb;   // staging plan (stage NULL: atomics)
    int64_t B; int64_t NU; int64_t NI;
    int D;
    float lr; float eps; float invB; float l2w; float a_w; float b_w;
    int sigmoid;                              // WRMF: PointwiseMSELoss(sigmoid=True), pointwise_mse_loss.py:24-25
    float* partial;                           // [nwaves][2]
    float* wpartial;                          // [nwaves][D] (GMF)
    int* err;
    // lazy TF-2.0 Adam: second slots, per-row step stamps (the bias shares its item row's), lr_t table
    float* a2U; float* a2V; float* a2b; int* lastU; int* lastV; int* lastb;
    const float* lrt; float b1; float b2; int step_t; int newton;
    const float4* lrv; float cf_delta, cf_lb1, cf_lb2;      // closed-form replay (orx_device.h AdamCF; NULL: the replay loops)
    // in-launch application of the PREVIOUS step's duplicated rows, as in the pairwise step (n_apply_blocks == 0: off): the first
    // blocks of the launch run inline_apply on `ap` (the tables seen as a pairwise step sees them, prev_* = step s-1's lists);
    // references marked urgent (bit 28 of the rewritten ids) wait for their row's ready flag
    int n_apply_blocks; int epoch; const int* readyU; const int* readyV;
    PairArgs ap;
    // pairing (round 6; kernels_plan.hip): the step's input records (user id, item id, label bits, pairing word | origin << 10), NULL: off
    const int4* ids4;
    // GMF, float4 kernels (round 6): the Dense(1) gradient is summed and its rule applied by wt_nred REDUCER workgroups at the end of the
    // launch itself (kernels_pointwise.hip dense_tail_reducer) instead of two more launches between this step and the next.  0: off
    int wt_nred;                              // orx_point_reducers(D, B)
    float* wt_rows;                           // [wt_nred - 1][D] the sums of 64 consecutive workgroups' partial rows (slots start out WT_EMPTY)
    float* wt_gout; float* wt_l2slot; float* wt_acc; int wt_optkind;      // as dense_reduce_kernel's arguments
};

int orx_launch_point_fused(orx_ctx* ctx, int model, int optkind, int mode, const PointArgs& a);
int orx_launch_dense_reduce(orx_ctx* ctx, const float* wpartial, int nwaves, int D, float* w, float l2w, float* gout,
                            float* l2slot, float* acc, int optkind /* -1: gradient to gout only */, float lr, float eps);
int orx_launch_dense_apply(orx_ctx* ctx, float* w, float* acc, float* g, int n, int optkind, float lr, float eps);
int orx_launch_score_all(orx_ctx* ctx, const float* U, const float* V, const float* b, const float* w,
                         const int32_t* uid, int64_t nq, int64_t NU, int64_t NI, int D, int kind, float* out);
int orx_point_nwaves(int D, int64_t B);
int orx_point_wparts(int D, int64_t B);
bool orx_point_dense_tail_ok(int D);
int orx_point_reducers(int D, int64_t B);
int orx_launch_score_mfma(orx_ctx* ctx, const float* U, const float* V, const float* b, const float* w, const int32_t* uid,
                          int64_t nq, int64_t NU, int64_t NI, int D, int kind, float* out, bool* launched);

// top-K selection (kernels_topk.hip)
struct TopkSelectArgs {
    // dense rows (scores != NULL): row r is scores[r ld + j], j < m, item id j;  candidates (cs != NULL): row q is
    // (cs, ci)[q C + i], i < cnt[q] (a row with cnt[q] > C overflowed and is left alone)
    const float* scores; int64_t ld; int64_t m;
    const float* cs; const int32_t* ci; int* cnt; int C;
    const int32_t* rowmap;                      // dense rows: the batch user of row r (NULL: r)
    const int64_t* eptr; const int32_t* eitems; // the users' sorted exclusion rows (eptr NULL: none)
    int k;
    int32_t* out_items; float* out_scores;      // [users][k]
    float* theta;                               // threshold mode: theta[q] (NaN: fewer than k eligible) and cnt[q] = 0 / C + 1
};
int orx_launch_topk_select(orx_ctx* ctx, const TopkSelectArgs& a, int64_t rows);      // one workgroup per row
constexpr int TOPK_FILTER_BLOCKS = 2048;   // most workgroups of one filter launch
constexpr int TOPK_POOL = 2048;            // pending candidates per workgroup (pool_iu / pool_s: TOPK_FILTER_BLOCKS x TOPK_POOL)
int orx_launch_topk_filter(orx_ctx* ctx, const float* U, const float* V, const float* b, const float* w, const int32_t* uid,
                           int64_t nq, int64_t NU, int64_t NI, int D, int kind, const float* theta, int* cnt, float* cs,
                           int32_t* ci, int C, int2* pool_iu, float* pool_s, bool* launched);

// launchers implemented in kernels_pairwise.hip
int orx_launch_dedup(orx_ctx* ctx, const DedupArgs& a, int64_t K);
int orx_launch_fused(orx_ctx* ctx, int model, int optkind, int mode, const PairArgs& a);
int orx_launch_fused_weighted(orx_ctx* ctx, int model, int optkind, int mode, const PairArgs& a);     // a.wt != NULL (kernels_pairwise_weighted.hip)
int orx_launch_hot_reduce(orx_ctx* ctx, const PairArgs& a, int level);

// host-side plan of the exact steps (api.hip), shared by the pairwise and the pointwise step
struct PairPlan { int nw; int64_t chunk; int64_t list_stride; int64_t Bp; int64_t item_stride; int tree_off[3];
                  int min_late = -1;      // staging plan from this many third-or-later references per range on (< 0: max(64, n / 512))
                  int pair_tpw = 0;       // pairing: triplets per wavefront of the fused kernel (0: off)
                  int64_t cap = 0; };     // steps the per-step scratch is sized for (>= chunk)
struct ExactChunk { bool hot = false, use_stage = false, dense_dups = false; int tree_levels = 0;
                    bool quiet = false; };      // the plan's counters were quiet (api.hip, "no read-back")
// pairing (kernels_plan.hip): is it on for a step of this form, and its per-call buffers (api.hip)
bool orx_pairing_wanted(int mode, bool role_bits, int optkind, int dim, int64_t B, int fb);
int orx_pairing_buffers(orx_ctx* c, int64_t B, int dim, PairPlan* plan);
int orx_exact_buffers(orx_ctx* c, orx_table* U, orx_table* V, int64_t K, int64_t B, int mode, bool role_bits,
                      bool inline_apply, bool staging, int nb_total, int nw, PairPlan* plan);
int orx_exact_plan_chunk(orx_ctx* c, orx_table* U, orx_table* V, const int32_t* uid, const int32_t* pid, const int32_t* nid, int64_t ds,
                         int64_t nU, int64_t nP, int64_t nN, int64_t kc, int64_t B, bool role_bits, bool inline_apply, bool staging,
                         const PairPlan& plan, ExactChunk* out, const std::function<int()>* while_waiting = nullptr);
// the same in two halves, for steps i0 .. i0 + kc - 1 of the chunk's plan arrays (bucketed plan only): issue enqueues the plan on the
// context's CURRENT stream and records `counters` after the read-back of the per-step counters; finish waits for it on the host
int orx_exact_plan_issue(orx_ctx* c, orx_table* U, orx_table* V, const int32_t* uid, const int32_t* pid, const int32_t* nid, int64_t ds,
                         int64_t nU, int64_t nP, int64_t nN, int64_t kc, int64_t B, bool inline_apply, bool staging,
                         const PairPlan& plan, int64_t i0, hipEvent_t counters, const std::function<int()>* after_readback = nullptr);
int orx_exact_plan_finish(orx_ctx* c, int64_t kc, int64_t B, bool inline_apply, bool staging, int64_t i0, hipEvent_t counters, ExactChunk* out, bool pairing_on = false);
// the DedupArgs of steps i0 .. of the chunk's plan arrays, as every exact step fills them (api.hip)
void orx_plan_dedup_args(orx_ctx* c, orx_table* U, orx_table* V, const int32_t* uid, const int32_t* pid, const int32_t* nid, int64_t ds,
                         int64_t nU, int64_t nP, int64_t nN, int64_t B, bool role_bits, bool inline_apply, bool staging,
                         const PairPlan& plan, int64_t i0, DedupArgs* out);
// geometry of the bucketed plan for d.{nU, nP, nN, NU, NI} and the constants of kernels_plan.hip (host only):
// {nru, nri, lgu, lgi, shift, W, PL_UN, PL_LCNT, PL_PAIR_CAP, ORX_SEG_DIRECT, ORX_PIECE, threads, threads of a big plan, PL_CHUNK}
void orx_plan_geometry_query(const DedupArgs& d, int32_t out[14]);
void orx_exact_step_views(orx_ctx* c, const PairPlan& plan, int64_t i, int64_t B, int D, bool use_stage, PairArgs* a);
int orx_launch_rows_planned(orx_ctx* ctx, int optkind, const RowsArgs& a);
// K id lists of n local rows each (ids [K][n], < 0 = padding) against ONE table: plan once (duplicate roles, staging
// plan, reduction tree), then per list i: orx_apply_rows_planned_step(i, grads).  SGD / Adagrad.
struct RowsPlan { PairPlan plan; ExactChunk ck; int64_t n = 0; bool ready = false; };
int orx_apply_rows_plan(orx_ctx* ctx, orx_table* t, const int32_t* ids, int64_t K, int64_t n, int64_t id_stride, RowsPlan* out);
int orx_apply_rows_planned_step(orx_ctx* ctx, orx_opt* opt, orx_table* t, orx_table* bias, const RowsPlan& rp, int64_t i,
                                const int32_t* ids, const float* grads, int64_t g_stride);
int orx_launch_dup_apply(orx_ctx* ctx, int optkind, const PairArgs& a);
bool orx_launch_tail(orx_ctx* ctx, int optkind, const PairArgs& a, const ReduceArgs& r, int64_t K, int* rc);     // dup_apply of the last step + loss_reduce in one launch
int orx_launch_urgent(orx_ctx* ctx, const DedupArgs& a, int64_t K);
// bucketed plan (kernels_plan.hip): same outputs as orx_launch_dedup (+ orx_launch_urgent) with `d` filled the same way
bool orx_plan_v2(bool role_bits);
int orx_plan_buffers(orx_ctx* c, int64_t chunk, int64_t B, int64_t NU, int64_t NI, bool want_dupbits);
int orx_launch_plan(orx_ctx* ctx, const DedupArgs& d, int64_t kc, bool keep_dupbits, int64_t step0 = 0);
int orx_launch_plan_urgent(orx_ctx* ctx, const DedupArgs& d, int64_t kc, int64_t step0 = 0);
int orx_launch_plan_swap(orx_ctx* ctx, const DedupArgs& d, int64_t kc);      // pairing: the records of the positions an accepted pair moves change places
int orx_fused_tpw(int D);                        // triplets per wavefront of the float4 fused kernel (0: generic dim)
int orx_fused_can_inline_apply(int D);
int orx_dedup_words(void);
int orx_launch_loss_reduce(orx_ctx* ctx, const ReduceArgs& a, int64_t K);
int orx_fused_nwaves(int D, int64_t B);
int orx_dedup_buckets(int64_t rows);
int64_t orx_dedup_range_rows();                  // rows per dedup range (one workgroup)

// fused-kernel modes
enum { MODE_EXACT = 0,     // unique rows in place; duplicate rows -> gsum, applied by dup_apply
       MODE_HOGWILD = 1,   // everything in place, racy, no duplicate handling
       MODE_ACCUM = 2,     // everything -> gsum (Adam: dense sweep follows)
       MODE_LOSS = 3 };    // forward only

// Internal model value of the pairwise kernels (not part of the public orx_pair_model): BPR without item biases
// (PairwiseLogLoss with p_item_bias = n_item_bias = None).  The score is u.p - u.n; no kernel built for it loads or stores
// b / gb / gb2 / ab / a2b / lastb / stageb / partb, which are NULL on this route.
enum { MODEL_BPR_NB = 16 };

// kernels_misc.hip
int orx_launch_init_uniform(orx_ctx* ctx, float* w, int64_t n, float lo, float hi, uint64_t seed);
int orx_launch_fill(orx_ctx* ctx, float* w, int64_t n, float v);
int orx_launch_gather(orx_ctx* ctx, const float* w, const float* bias, int64_t rows, int dim,
                      const int32_t* ids, int64_t n, float* out, int64_t out_stride, int* err,
                      int skip_negative = 0, float* bias_out = nullptr);   // bias_out: the biases go there ([n]) instead of column dim of out
int orx_launch_censor(orx_ctx* ctx, float* w, const unsigned char* dflag, int64_t rows, int dim, const int32_t* ids,
                      int64_t n, float min_norm, int* err);
int orx_launch_censor2(orx_ctx* ctx, float* wA, const unsigned char* fA, int64_t rowsA, const int32_t* idsA, int64_t nA,
                       float* wB, const unsigned char* fB, int64_t rowsB, const int32_t* idsB, int64_t nB,
                       int dim, float min_norm);
int orx_launch_adam_sweep(orx_ctx* ctx, float* w, float* m, float* v, float* gsum, int64_t n,
                          float lr_t, float b1, float b2, float eps);

// kernels_dense.hip (DLRM dense side)
int orx_launch_gemm(orx_ctx* ctx, const float* A, int64_t sa0, int64_t sa1, const float* B, int64_t sb0, int64_t sb1,
                    float* C, int64_t ldc, const float* bias, int M, int N, int K, int act, bool c_zero = false, float out_scale = 1.0f);
int orx_launch_gemm_f16(orx_ctx* ctx, const float* A, int64_t sa0, int64_t sa1, const float* B, int64_t sb0, int64_t sb1,
                        float* C, int64_t ldc, const float* bias, int M, int N, int K, int act, bool c_zero = false, float out_scale = 1.0f);
struct DenseParam { float* w; float* acc; float* acc2; float* g; int64_t n; };
int orx_launch_dense_apply_multi(orx_ctx* ctx, const DenseParam* ps_dev, int count, int64_t max_n, int optkind, float lr, float eps,
                                 float b1 = 0.f, float b2 = 0.f);
// the same rule in 64 x 64 tiles, with the rest of a dense parameter's per-step work folded in: the split-K slices of its gradient
// (kernels_gemm16.hip) are added on the way in (slice order; times slab_scale = 1 / loss scale), the fp16 copies of the new weights
// (w16 [rows][ld16], w16t [cols][ld16t], transposed through LDS) are written on the way out
struct DenseFused {
    float* w; float* acc; float* acc2; float* g; int rows, cols;
    const float* slab; int S, ntn;                 // NULL: the gradient is g alone
    void* w16; void* w16t; int ld16, ld16t;        // NULL: no fp16 copies
    int tile0, tiles_x;                            // first tile of this parameter in the launch's flat tile list; tiles per tile row
    const float* cparts; int cN;                   // a vector parameter (rows == 1 or cols == 1) whose gradient arrives as partial rows [P][cN]
                                                   // (ColPart): added here in colparts_reduce_kernel's order -- no reduce launch (round 6)
};
// first tile of every parameter, and how many partial rows its gradient has THIS step (0: none) -- kernel arguments
struct DenseFusedTiles { int count; int tile0[48]; int cP[48]; };
struct CsrFinish;       // (orx_csr_device.h) the sorted sparse apply's finish pass, carried by the dense optimizer's launch
int orx_launch_dense_apply_fused(orx_ctx* ctx, const DenseFused* ps_dev, const DenseFusedTiles& tt, int total_tiles, int optkind, float lr, float eps,
                                 float b1, float b2, float slab_scale, const CsrFinish* finish = nullptr);
// orx_csr_apply without its second launch: the blocks' sums + rule are launched, the finish pass is DESCRIBED (*finish) for a launch that takes it along
int orx_csr_apply_split(orx_ctx* ctx, orx_opt* opt, orx_table* t, const uint2* sorted, int64_t n, const float* grads, int64_t g_stride,
                        bool skip_single, CsrFinish* finish);
// Column sums (bias gradients) leave their producers as one partial row per row block -- parts[p * N + c], plain stores --
// and one colparts_reduce launch per MLP backward adds the blocks in order: no fp32 atomics, reproducible sums.
struct ColPart { float* parts = nullptr; int P = 0; };        // in: the workspace; out: row blocks written
struct ColJob { const float* parts; float* out; int N, P; float scale; };     // out = scale * sum of the partial rows
constexpr int ORX_COLJOBS_MAX = 24;
struct ColJobs { ColJob j[ORX_COLJOBS_MAX]; };
int orx_launch_colparts_reduce(orx_ctx* ctx, const ColJob* jobs, int n);
int orx_launch_act_bwd_colsum(orx_ctx* ctx, float* dY, const float* Y, int64_t ldy, int M, int N, int act, ColPart* gb,
                              void* d16 = nullptr, int64_t ld16 = 0, const float* src = nullptr, int64_t ld_src = 0, float src_scale = 1.0f);
int orx_launch_gemm_f16s(orx_ctx* ctx, const void* A16, int64_t lda, const void* B16, int64_t ldb, float* C, int64_t ldc,
                         void* C16, int64_t ldc16, const float* bias, int M, int N, int K, int act,
                         const float* actY = nullptr, int64_t ldy = 0, int act_y = 0, ColPart* gb = nullptr);
// second-generation fp16 products (kernels_gemm16.hip): C = A16 * B16^T on K-contiguous fp16 operands with the fused epilogues,
// and the weight gradient C += A16^T * B16 from batch-major fp16 copies (split-K through fp32 slabs + one reduce launch)
bool orx_gemm16_nt_ok(int64_t lda, int64_t ldb, int N, int K);
int orx_launch_gemm16_nt(orx_ctx* ctx, const void* A16, int64_t lda, const void* B16, int64_t ldb, float* C, int64_t ldc,
                         void* C16, int64_t ldc16, const float* bias, int M, int N, int K, int act,
                         const float* actY = nullptr, const void* actY16 = nullptr, int64_t ldy = 0, int act_y = 0, ColPart* gb = nullptr,
                         // relu masks (kernels_gemm16.hip Nt16Args): written by a relu layer's forward launch, read by the input-gradient launch above it
                         unsigned long long* mask_out = nullptr, const unsigned long long* mask_in = nullptr);
int orx_gemm16_nt_config(orx_ctx* ctx, int M, int N, int64_t* words_out);
// What the launchers choose for a shape on `num_cu` CUs (host code; the launchers and the query orx_gemm16_plan call these):
//   nt: cfg 1 = 256 x 128, 2 = 128 x 128, 3 = 128 x 64; stages 0 = register-staged, 2 / 3 = LDS-DMA; wave_tile 64 / 128; tail = the TAIL form
struct Nt16Plan { int cfg, stages, wave_tile, tail, bm, bn, threads; int64_t blocks, mask_words; };
Nt16Plan orx_gemm16_nt_plan(int num_cu, int M, int N, int64_t lda, int64_t ldb);
//   tn: the split (S slices of kchunk samples over `tiles` tiles); form 0 = register-staged, 2 / 3 = LDS-DMA, 4 = two K groups; tail
struct Tn16Plan { int S, tiles, kchunk, form, tail; };
Tn16Plan orx_gemm16_tn_form(int num_cu, int M, int N, int K, int64_t lda, int64_t ldb);
//   grouped launch of a layer [B, out] -> [B, in]: would the DLRM step group it, the grid's two parts, the two TAIL flags
struct Group16Plan { int grouped, tn_tail, nt_tail, S, tiles, kchunk, n_tn, n_nt; };
Group16Plan orx_gemm16_group_plan(int num_cu, int B, int in, int out, int64_t ldx, int64_t lddz, int64_t ldw, int nt_cols);
#define ORX_SLAB_STRIDE (128 * 128 + 64)          // floats per (tile, slice) of a split-K workspace (kernels_gemm16.hip)
struct SlabReduce { const float* slab; float* C; int64_t ldc; int M, N, S, ntn, tiles; };
bool orx_gemm16_tn_ok(int64_t lda, int64_t ldb, int N);
void orx_gemm16_tn_plan(orx_ctx* ctx, int M, int N, int K, int* S_out, int* tiles_out, int* kchunk_out);
int orx_launch_gemm16_tn(orx_ctx* ctx, const void* A16, int64_t lda, const void* B16, int64_t ldb, float* C, int64_t ldc,
                         float* slab, int M, int N, int K, float out_scale = 1.0f);
int orx_launch_slab_reduce(orx_ctx* ctx, const void* jobs_dev, int n_jobs, int max_tiles, float out_scale = 1.0f);
// the weight gradient (arguments of orx_launch_gemm16_tn) and the input gradient (of orx_launch_gemm16_nt) of one layer in ONE launch
bool orx_gemm16_group_ok(orx_ctx* ctx, int B, int in, int out, int64_t ldx16, int64_t ldw16);
int orx_launch_gemm16_group(orx_ctx* ctx, const void* X16, int64_t ldx, const void* dZ16, int64_t lddz, float* gW, int64_t ldgw, float* slab,
                            int in, int out, int B, float out_scale,
                            const void* W16, int64_t ldw, float* C, int64_t ldc, void* C16, int64_t ldc16,
                            const float* actY, const void* actY16, int64_t ldy, int act_y, ColPart* gbp, const unsigned long long* mask_in = nullptr,
                            int nt_cols = 0);     // > 0: the input-gradient product's column count (the weight operand padded with zero rows)
int orx_launch_cast16(orx_ctx* ctx, const float* src, int64_t lds_, void* dst16, int64_t ld16, int M, int N);
bool orx_head16_ok(int K, int64_t ldx);
int orx_launch_head_fwd(orx_ctx* ctx, const void* X16, int64_t ldx, const void* w16, const float* bias, int act, float* pred, int B, int K);
// hl != NULL: the loss is folded into the head's backward (no dlrm_loss_kernel launch): dy is formed from pred and the label, the loss
// terms leave as one fp64 partial per workgroup in loss_part[0 .. orx_head_bwd_blocks(B))
struct HeadLoss { const float* label; int bce; float thr; int64_t n_mean; float gscale; double* loss_part;
                  const float* fwd_bias; float* pred_out; };       // fwd_bias != NULL: head_bwd_kernel runs the head's forward as well (pred -> pred_out)
int orx_launch_head_bwd(orx_ctx* ctx, const void* X16, int64_t ldx, const void* w16, const float* dy, const float* pred, int act, int act_below,
                        ColPart* gW, ColPart* gb, void* dZ16, int64_t ld16, float* dZ32, int64_t ld32, ColPart* gb_below, int B, int K,
                        const HeadLoss* hl = nullptr);
int orx_head_bwd_blocks(orx_ctx* ctx, int B);
int orx_launch_head_loss_finish(orx_ctx* ctx, const double* parts, int64_t stride, int n, int64_t K, int64_t n_mean, double* loss_out);
struct ShadowParam { const float* w; void* w16; void* w16t; int in, out, ld16, ld16t; };
int orx_launch_dense_shadow(orx_ctx* ctx, const ShadowParam* ps_dev, int count, int64_t max_n);
int orx_launch_act_bwd(orx_ctx* ctx, float* dY, const float* Y, int64_t ldy, int M, int N, int act);
int orx_launch_copy2d(orx_ctx* ctx, float* dst, int64_t ldd, const float* src, int64_t lds_, int M, int N, float scale = 1.0f);
int orx_launch_interact(orx_ctx* ctx, bool fwd, const float* Z, const float* dR, int F, int d, int compat, int itself,
                        float* out, int P, int64_t B, int ldR, void* R16 = nullptr, int ldR16 = 0, bool* wrote16 = nullptr,
                        const float* emb = nullptr, const int32_t* idx = nullptr, int64_t emb_rows = 0, float scale = 1.0f,
                        float* gdst = nullptr,
                        // backward with direct rows: flags [B][F] of the lookups whose row nobody else references in the step -- their
                        // SGD / Adagrad update is applied in place by the kernel (kernels_dense.hip FusedRows), no gradient row is written
                        const unsigned char* single = nullptr, int opt_kind = 0, float lr = 0.f, float eps = 0.f, float* acc_rows = nullptr);
bool orx_interact_direct_ok(int F, int d, int compat);
bool orx_interact_fuse_ok(int F, int d, int compat);
int orx_launch_dlrm_loss(orx_ctx* ctx, float* P, const float* y, int64_t B, int bce, float thr, float* dP, double* loss_out,
                         int64_t n_mean = 0, int accumulate = 0, float gscale = 1.0f);
int orx_launch_dlrm_tiny_apply(orx_ctx* ctx, const int32_t* idx, const float* dZ, const int* tiny_f_dev, int n_tiny, int max_rows,
                               const int64_t* offset, const int64_t* rows, int F, int d, int64_t B, float lr, float* W);
int orx_launch_dlrm_mask_tiny(orx_ctx* ctx, const int32_t* idx, const unsigned char* is_tiny_dev, int F, int64_t total, int32_t* out);
int orx_launch_dlrm_ids(orx_ctx* ctx, const int32_t* sparse, const int64_t* offset, const int64_t* rows, int nf, int64_t B,
                        int32_t* idx);
int orx_launch_rows_accum(orx_ctx* ctx, float* G, const int32_t* ids, const float* grads, int64_t g_stride, int64_t n, int D, int64_t rows);

// kernels_rowsort.hip: deterministic apply of per-occurrence gradient rows (stable sort by row + segmented sums in position order)
int orx_rows_sort(orx_ctx* ctx, const int32_t* ids, int64_t K, int64_t n, int64_t id_stride, int64_t rows, const uint2** sorted);
int orx_rows_sort_reserve(orx_ctx* ctx, int64_t K, int64_t n, int64_t rows);
int orx_csr_apply(orx_ctx* ctx, orx_opt* opt, orx_table* t, const uint2* sorted, int64_t n, const float* grads, int64_t g_stride,
                  bool skip_single = false);       // skip_single: rows referenced once were updated by the kernel that formed their gradient
int orx_rows_single_flags(orx_ctx* ctx, const uint2* sorted, int64_t K, int64_t n, int64_t rows, unsigned char* flags);
int orx_csr_accum(orx_ctx* ctx, orx_table* t, const uint2* sorted, int64_t n, const float* grads, int64_t g_stride);
int orx_csr_accum_into(orx_ctx* ctx, float* G, int64_t rows, int dim, const uint2* sorted, int64_t n, const float* grads, int64_t g_stride);
int orx_csr_adam(orx_ctx* ctx, bool step, const AdamRowsArgs& r, orx_table* t, const uint2* sorted, int64_t n);
int orx_adam_rows_sorted(orx_ctx* ctx, orx_opt* opt, orx_table* t, const uint2* sorted, int64_t n, const float* grads, int64_t g_stride, bool step);
int orx_adam_dense_sorted(orx_ctx* ctx, orx_opt* opt, orx_table* t, const uint2* sorted, int64_t n, const float* grads, int64_t g_stride);

// device-side exchange plan of the sharded step (kernels_sharded.hip)
struct RouteArgs {
    const int32_t* uid; const int32_t* pid; const int32_t* nid; int64_t B;
    int world; int cap;
    int32_t* send;           // [world*cap][3], pre-filled with -1
    int* counters;           // [world], zeroed
    int* overflow; int* err;
    int64_t NU, NI;          // GLOBAL table rows (id validation)
    int64_t id_stride;       // K-step launch (grid.y = step): ids of step k at + k*id_stride, send / counters of step k
                             // at + k*world*cap*3 / + k*world
};

struct RequestArgs {
    const int32_t* trip;     // [T][3] received triplets, u < 0 = empty slot
    int64_t T; int world; int cap;
    int32_t* send_ids;       // [world*cap], pre-filled with -1
    int32_t* slot;           // [2T]: slot of the p / n request of triplet t, -1 if none
    int32_t* u_loc;          // [T]: local user row or -1
    int* counters;           // [world], zeroed
    int* overflow;
    // K-step launch (grid.y = step): every array of step k at + k * (its per-step size)
    // hot-item replication (0: off): items 0 .. hot-1 live in a replica on every rank -- their references ask nobody.
    // They take slots world * cap .. world * cap + cap_hot - 1 (the region BEHIND the exchanged buckets in the row / gradient buffers)
    // and leave their ids in hot_ids [cap_hot] (pre-filled with -1); counters then has world + 1 entries per step
    int hot; int cap_hot; int32_t* hot_ids;
};

struct ShardGradArgs {
    const float* U;          // local user shard [rows, D]
    const float* rows_in;    // [world*cap2][DS] received item rows, bias at column D
    const int32_t* u_loc;    // [T]
    const int32_t* slot;     // [2T]
    float* gu;               // [T][D]
    float* send_g;           // [world*cap2][DS]
    int64_t T; int D; int DS;
    float invB; float margin; float l2w;
    float* partial;
    // SGD with the user apply folded in (orx_shard_grads_sgd): duplicate flags of the u_loc list, writable table, rate,
    // and the id list left for the flagged apply of the duplicated rows (-1: already applied)
    const unsigned char* fu; float* Uw; float lr; int32_t* u_apply;
    // per-destination dedup of the requests (orx_shard_request_dedup_steps): references that share a slot add their gradients
    // into it (send_g zeroed by the caller); NULL: every reference has a slot of its own
    const unsigned char* dupref;   // [2T]
    float* gdup;                   // [2T][DSg] side buffer: gradients of the references that share a slot (row = reference index)
    // the bias apart from the rows (the sharded engine's exchange carries it as a message of its own: D + 1 floats per row on the
    // wire instead of D + 4): received biases [world*cap2], bias gradients out [world*cap2]; rows_in / send_g rows are then DS = D floats
    const float* bias_in; float* gb_out; int DSg;   // DSg: row stride of gdup (D + 4; its column D is the bias gradient)
};

struct DedupReqArgs {
    const int32_t* trip;     // [K][T][3]
    int64_t T; int world; int cap; int64_t Lr;     // Lr = rows of the item table per rank (ceil(items_global / world))
    int32_t* keys;           // [K][2T] scratch: owner * Lr + local row of every item reference (p refs, then n refs), -1 dead
    const uint2* sorted;     // [K][2T] (key, reference) ascending
    int32_t* uq;             // [K][2T] scratch
    int* chunkcnt; int nchunk;  // [K][nchunk] heads per chunk of 1024 sorted entries, then their exclusive prefix
    int* ostart;             // [K][64] index (among the list's distinct keys) of every owner's first key
    int2* seglist; int* segcount;   // [K][T] (slot, first sorted entry) of the shared slots, [K] their number (NULL: not wanted)
    int32_t* send_ids; int32_t* slot; int32_t* u_loc; unsigned char* dupref; int* overflow;
};
int orx_launch_shard_keys(orx_ctx* ctx, const DedupReqArgs& a, int64_t K);
int orx_launch_shard_dedup_slots(orx_ctx* ctx, const DedupReqArgs& a, int64_t K);
int orx_shard_grads_impl(orx_ctx* ctx, int model, orx_opt* opt, orx_table* user, const float* rows_in, const float* bias_in,
                         const int32_t* u_loc, const int32_t* slot, const uint8_t* dupref, const void* sorted, const void* seglist,
                         const int32_t* segcount, float* gdup, const uint8_t* dup_u, int64_t T, int64_t row_stride, int64_t B_global,
                         float margin, int flags, float* gu, int32_t* u_apply, float* send_g, float* gb_out, double* loss_l2_accum,
                         float* partial_ext = nullptr, int* nwaves_out = nullptr);
int orx_apply_rows_flagged_impl(orx_ctx* ctx, orx_opt* opt, orx_table* t, orx_table* bias, const int32_t* ids, int64_t n,
                                const float* grads, int64_t g_stride, const float* gbias, const unsigned char* dflag);
// two flagged SGD lists (tables of one dim) in one launch where that applies, else one after the other
int orx_apply_rows_flagged_pair(orx_ctx* ctx, orx_opt* opt, orx_table* tA, orx_table* biasA, const int32_t* idsA, int64_t nA, const float* gA, int64_t strideA,
                                const float* gbiasA, const unsigned char* flagA, orx_table* tB, orx_table* biasB, const int32_t* idsB, int64_t nB, const float* gB,
                                int64_t strideB, const float* gbiasB, const unsigned char* flagB, bool flags_over_both = false);
int orx_launch_shard_segsum(orx_ctx* ctx, const int2* seglist, const int* segcount, const uint2* sorted, int64_t n, const float* gdup, int DSg,
                            float* send_g, int DS, int D, float* gb_out);
int orx_launch_shard_route(orx_ctx* ctx, const RouteArgs& a, int64_t K = 1);
int orx_launch_shard_request(orx_ctx* ctx, const RequestArgs& a, int64_t K = 1);
int orx_launch_shard_hot_pack(orx_ctx* ctx, float* gV, float* gb, float* hg, int64_t H, int D, int DSh);      // hot-item replication: scratch sums -> [H][D + 4] block
int orx_launch_shard_bucket(orx_ctx* ctx, const int32_t* ids, int64_t n, int world, int cap, int32_t* send_ids, int32_t* slot,
                            int* counters, int* overflow);
int orx_launch_shard_localize(orx_ctx* ctx, const int32_t* ids, int64_t n, int world, int32_t* out);
int orx_launch_shard_grads(orx_ctx* ctx, int model, const ShardGradArgs& a, int* nwaves);

// kernels_eval.hip (ranking metrics of the evaluation step)
struct EvalArgs {
    const float* pred;            // [n, NI]
    const unsigned char* pos;     // [n, NI]
    const unsigned char* excl;    // [n, NI]
    int64_t NI;
    const float* at; int nat;     // cut-offs
    float* auc; float* ndcg; float* recall;   // [n], [n, nat], [n, nat]
    int* err;
};
int orx_launch_rank_metrics(orx_ctx* ctx, const EvalArgs& a, int64_t n);
struct EvalCsrArgs {
    const float* pred;            // [n, NI]
    unsigned* pbits; unsigned* ebits;                 // [n, W] bitmaps built from the lists (ebits = pbits + n W)
    const int64_t* pos_ptr; const int32_t* pos_items; // CSR over the n users of the call
    const int64_t* excl_ptr; const int32_t* excl_items;
    int64_t NI, W;
    const float* at; int nat;
    float* auc; float* ndcg; float* recall;
    unsigned* part; int* neval; int S; int* flag_out;
    int64_t q0;                                       // first user of this launch (slices of the batch)                // per-(user, segment) partial counts [n][S][136]; evaluated items per user
    int* err;
};
int orx_rank_csr_segments(int64_t n, int64_t NI);
int orx_launch_mask_bits(orx_ctx* ctx, const EvalCsrArgs& a, int64_t n, int clear);
int orx_launch_rank_sweeps(orx_ctx* ctx, const EvalCsrArgs& a, int64_t q0, int64_t nq, int64_t max_pos);

// the same metrics without the score matrix (kernels_evalmf.hip): one batch of nq users
struct EvalMfArgs {
    const float* U; const float* V; const float* b; const float* w;
    const int32_t* uid; int64_t nq; int64_t NU; int64_t NI;
    int D; int Dp; int TI; int64_t chunk;
    const int64_t* pos_ptr; const int32_t* pos_items;     // CSR over the batch's users, offsets from 0, rows strictly ascending
    const int64_t* excl_ptr; const int32_t* excl_items;
    float* pos_s; float* excl_s;                          // the listed items' scores, entry for entry
    float* ts; int* tex; int NB;                          // [nq][NB] the chunk's sorted thresholds (ts[0] = -inf) and their "excluded" flags
    unsigned* hist; unsigned* corr; unsigned* nzdrop;     // [nq][NB] | [nq][NB] (one piece) and [nq]: the chunk's counts over ALL items
    const float* at; int nat;
    float* auc; float* ndcg; float* recall; int* neval;
    int* err;
};
bool orx_evalmf_has_tile(int D);
int orx_launch_evalmf_gather(orx_ctx* ctx, const EvalMfArgs& a, int kind, int64_t max_list);
int orx_launch_evalmf_chunk(orx_ctx* ctx, const EvalMfArgs& a, int kind, int c0, int last);

// scores and metrics of candidate lists (kernels_cand.hip): one batch of nq users, flat lists with offsets from 0
struct CandScoreArgs {
    const float* U; const float* V; const float* b; const float* w;
    const int32_t* uid; int64_t nq; int D;
    const int64_t* ptr; const int32_t* items; int64_t E;  // E = ptr[nq] entries, ids checked on the host
    float* out;                                           // [E] entry for entry
};
struct CandRankArgs {
    const int64_t* pos_ptr; const int32_t* pos_items; const float* pos_s;       // rows strictly ascending
    const int64_t* cand_ptr; const int32_t* cand_items; const float* cand_s;
    int NB;                                               // 2^STEPS from the call's longest positive list, as rank_sweep_kernel picks it
    const float* at; int nat;
    float* auc; float* ndcg; float* recall;
};
bool orx_cand_has_tile(int D);
int orx_launch_cand_score(orx_ctx* ctx, const CandScoreArgs& a, int kind);
int orx_launch_cand_pick(orx_ctx* ctx, const float* rows, int64_t NI, const int64_t* ptr, const int32_t* items, int64_t nq,
                         int64_t E, float* out);
int orx_launch_cand_rank(orx_ctx* ctx, const CandRankArgs& a, int64_t nq);

// kernels_sampler.hip (on-device triplet sampler); filled by sampler_args of api_sampler.hip and nowhere else
struct SamplerArgs {
    const int32_t* rec_user; const int32_t* rec_item; int64_t R;      // interaction records
    const int64_t* ptr; const int32_t* items;                          // CSR of positives (sorted per user)
    int64_t total_items; int64_t total_users;
    uint64_t seed; int64_t first; int64_t n; int h;
    int32_t* uid; int32_t* pid; int32_t* nid;
    const uint2* prop = nullptr;                                       // alias table of the negatives' proposal, (thr, alias) per item; NULL: uniform
};
int orx_launch_sample_pairwise(orx_ctx* ctx, const SamplerArgs& a);
int orx_launch_sample_stratified(orx_ctx* ctx, const SamplerArgs& a, float pos_ratio, float* label, int* blockcnt, int64_t* blockbase,
                                 int64_t* counter);
int orx_launch_sample_perpos(orx_ctx* ctx, const SamplerArgs& a, int nneg, float* label);
// out[i] = rec_w[record of sample a.first + i] (the positives' permutation of sample_pairwise_kernel); reads a.R, a.h, a.seed, a.first, a.n
int orx_launch_sample_weights(orx_ctx* ctx, const SamplerArgs& a, const float* rec_w, float* out);
// the first M candidates of orx_launch_hardneg for every sample, a.nid [n * M]; no table is read
int orx_launch_sample_multi(orx_ctx* ctx, const SamplerArgs& a, int M);

// the sampler object (api_sampler.hip creates it and holds every call on it)
struct orx_sampler {
    orx_ctx* ctx = nullptr;
    int32_t *rec_user = nullptr, *rec_item = nullptr, *items = nullptr;
    int64_t* ptr = nullptr;
    int64_t R = 0, total_users = 0, total_items = 0;
    int h = 1;
    // stratified pointwise stream: positives consumed so far (device), next sample index and seed the counter belongs to
    int64_t* d_counter = nullptr; int64_t strat_next = -1; uint64_t strat_seed = 0;
    int* d_blockcnt = nullptr; int64_t* d_blockbase = nullptr; size_t block_cap = 0;
    // proposal of the negatives: [total_items] records (thr, alias), allocated by the first orx_sampler_set_proposal
    uint2* d_prop = nullptr; bool prop_on = false;
    // per-record weights: [R] in the records' order, allocated by the first orx_sampler_set_record_weights
    float* d_recw = nullptr; bool recw_on = false;
    // WARP's trial-weight table: the device copy and the host floats it holds, uploaded only when they change
    float* d_warpw = nullptr; float h_warpw[256]; int warpw_n = 0;
};

// kernels_hardneg.hip (orx_sampler_pairwise_hard): the pairwise draw of `s` plus M candidates per sample, scored against the tables
struct HardNegArgs {
    SamplerArgs s;
    const float* U; const float* V; const float* b;       // b NULL: no item bias
    int model; int D; int M;
    int32_t* cand; float* cand_score;                     // [n * M] or NULL
};
int orx_launch_hardneg(orx_ctx* ctx, const HardNegArgs& a);

// kernels_multineg.hip (orx_multineg_step / orx_multineg_loss): one step's gradient launch of a positive against N negatives
struct MultiNegArgs {
    const float* U; const float* V; const float* b;       // read only; b NULL: no item bias
    const int32_t* uid; const int32_t* pid; const int32_t* nid;   // this step's ids: [B], [B], [B][N]
    const float* wt; const float* off;                    // [B] weights (NULL: all ones), [B][N] offsets of the negative logits (NULL: 0)
    float* gu; float* gi; int32_t* list;                  // [B][gs]; [(1 + N) B][gs], bias gradient in column D; [(1 + N) B] item ids
    int64_t B; int64_t NU; int64_t NI;
    int N; int D; int gs;
    float invB; float l2w;
    float* partial;                                       // [orx_multineg_nwaves(ctx, D, B)][2] loss / l2 partials of this step
    int* err;
};
int orx_multineg_nwaves(orx_ctx* ctx, int D, int64_t B);
int orx_launch_multineg(orx_ctx* ctx, int kind /* orx_multineg_kind */, bool grads, const MultiNegArgs& a);

// kernels_bag.hip (orx_bag_pool / orx_seqrec_step / orx_seqrec_loss): pooling of ragged item lists, one wavefront per bag, and the
// two kernels between the gradient launch and the sorted apply of the history table
struct BagArgs {
    const float* H; int64_t rows; int D;                  // the table the lists index
    const int32_t* ptr; const int32_t* items;             // DEVICE [B + 1] offsets, [n] ids
    int64_t B; int64_t n;
    int mode; float inv_denom;                            // orx_bag_mode; 1.0f / denom (ORX_BAG_FIXED)
    float* out;                                           // [B][D] q_i, rows of the call's first bag on
    int32_t* uid; float* coef; int32_t* owner;            // the step's (NULL: not kept): [B] i or -1 (a dead bag), [B] c_i (0: dead or empty), [n] the bag of a list position
    int* err;
};
int orx_launch_bag_pool(orx_ctx* ctx, const BagArgs& a);
int orx_launch_bag_scale_rows(orx_ctx* ctx, float* g, const float* coef, int64_t B, int D, int gs);           // g[i][0 .. D) *= coef[i]
int orx_launch_bag_owner_pairs(orx_ctx* ctx, const uint2* sorted, const int32_t* owner, int64_t n, int64_t B, uint2* out);   // (row, position) -> (row, owner[position])
// what the calls over bags share (api_seqrec.hip; api_tower.hip): the checks of the lists before any device work (host lists are
// walked); the scratch of the lists behind whatever the caller has carved -- ORX_BAG_STAGED: the pieces host lists are copied
// into, nothing else; ORX_BAG_FORWARD: + uid'; ORX_BAG_STEP: + c_i, the owners and the pairs the apply takes --; the kernels'
// arguments on d_tmp once it is grown (host lists are copied here; `out` is the caller's to set); the touch of the lazy rows of H
// on the sorted list, *sorted the pairs for a caller that applies with them
enum { ORX_BAG_STAGED = 0, ORX_BAG_FORWARD = 1, ORX_BAG_STEP = 2 };
struct BagLayout { size_t uid, ptr, items, coef, owner, pairs; int keep; };
int orx_bag_check(const char* fn, const int32_t* bag_ptr, const int32_t* bag_items, int64_t B, int64_t n, int mode, float denom, bool host);
void orx_bag_layout(Carve* cv, int64_t B, int64_t n, bool host, int keep, BagLayout* l);
int orx_bag_bind(orx_ctx* c, const BagLayout& l, orx_table* H, const int32_t* bag_ptr, const int32_t* bag_items, int64_t B, int64_t n, int mode,
                 float denom, bool host, BagArgs* a, uint2** pairs);
int orx_bag_stage(orx_ctx* c, const int32_t* bag_ptr, const int32_t* bag_items, int64_t B, int64_t n, bool host, int32_t* d_ptr, int32_t* d_items,
                  BagArgs* a);
int orx_bag_touch(orx_ctx* c, orx_table* H, const int32_t* items, int64_t n, bool always, const uint2** sorted);
// The history side of a step, in its two halves.  First: the lazy rows of H are touched on the sorted list, `launch` produces what
// the bags pool into (orx_launch_bag_pool, orx_launch_tower_input), and -- pairs not NULL: H is trained -- the sorted pairs'
// positions are replaced by their owners right away, before anything else may sort.  pairs NULL (a forward, or H outside the
// mask and so current): the touch alone, no sort unless H is lazy.  Second, after the counter has advanced: columns
// [col0, col0 + D) of the gradient rows g [B][ld] are scaled by c_i in place and orx_apply_rows_sorted sums a row's occurrences
int orx_bag_produce(orx_ctx* c, orx_table* H, const BagArgs& bag, uint2* pairs, const std::function<int()>& launch);
int orx_bag_apply(orx_ctx* c, orx_opt* opt, orx_table* H, const BagArgs& bag, const uint2* pairs, float* g, int col0, int ld);

// kernels_inbatch.hip (orx_inbatch_step / orx_inbatch_loss): one step of the in-batch softmax.  Bp = B rounded up to 64, Dp = D
// rounded up to 16; every [Bp] / [Bp][Dp] / [nch][..] array is scratch carved from the context's d_tmp
struct InBatchArgs {
    const float* U; const float* V; const float* b;       // read only; b NULL: no item bias
    const int32_t* uid; const int32_t* pid;               // this step's ids [B]
    const float* wt; const float* off;                    // [B] weights (NULL: all ones), [B] column offsets (NULL: 0)
    int64_t B; int64_t Bp; int64_t NU; int64_t NI;
    int D; int Dp; int gs; int nch; int tpc; int mask;    // nch column chunks of tpc tiles of 64; mask: ORX_IB_MASK_HITS
    float scale; float invB; float l2w;
    float* xu; float* xv;                                 // [Bp][Dp] the gathered rows
    int32_t* key; float* cb; float* co; float* cw; float* sq;     // [Bp] pid or -1, bias, offset, w / B, |u|^2 + |v|^2
    float* pm; float* pe; float* psd;                     // [nch][Bp] the chunks' running maximum, off-diagonal sum, diagonal score
    float* rmax; float* cn; float* dcoef; float* rowloss; // [Bp] the row maximum m_i (+inf: a dead row), c_i / tot_i, -c_i A_i, l_i
    float* gpu; float* gpv; float* bpart;                 // [nch][Bp][Dp] partial gradient tiles of the two sides, [nch][Bp] of the bias
    float* gu; float* gi;                                 // [B][gs] gradient rows, the bias gradient in column D of gi
    float* partial;                                       // [orx_inbatch_npartials(B)][2] loss / l2 partials of this step
    int* err;
};
inline int orx_inbatch_npartials(int64_t B) { return (int)((((B + 63) & ~(int64_t)63) + 255) / 256); }
void orx_inbatch_plan(int64_t B, int32_t D, int32_t chunk_cols, int32_t out[4], int* tiles_per_chunk = nullptr);
int orx_launch_inbatch_forward(orx_ctx* ctx, const InBatchArgs& a);     // gather, LSE pass, finalize
int orx_launch_inbatch_grads(orx_ctx* ctx, const InBatchArgs& a);       // the two gradient walks, the finishing pass

// kernels_fullsoftmax.hip (orx_fullsoftmax_step / orx_seqrec_full_step and their forwards): one step of the softmax over all
// items.  Bp = B and NIp = NI rounded up to 64, Dp = D rounded up to 16; every [Bp] / [NIp] / [..][Dp] / [chunks][..] array is
// scratch carved from the context's d_tmp
struct FullSoftmaxArgs {
    const float* Q; const float* V; const float* b;       // read only; Q [NQ][D]: the user table, or the pooled rows; b NULL: no item bias
    const int32_t* qid; const int32_t* pid;               // this step's [B] rows of Q (SeqRec form: i, -1 for a dead bag) and labels
    const float* wt; const float* off;                    // [B] weights (NULL: all ones), DEVICE [NI] item offsets (NULL: 0)
    int64_t B; int64_t Bp; int64_t NQ; int64_t NI; int64_t NIp;
    int D; int Dp; int gs; int nci; int tpi; int ncs; int tps;    // nci item chunks of tpi tiles of 64; ncs sample chunks of tps tiles
    float scale; float invB; float l2w;
    float l2q; const float* X0; int x0w; int x0ld;        // the query side's own l2: g_u takes l2q * u_i (orx_fullsoftmax_bind: l2w), and the l2 sum
                                                          // |u_i|^2 -- or, X0 not NULL, |X0[i][0 .. x0w)|^2 in its place (the tower: x0, with l2q = 0)
    float* xq; float* xv;                                 // [Bp][Dp] the query rows, [NIp][Dp] the zero-padded item table
    int32_t* key; float* cw; float* sq;                   // [Bp] pid or -1, w / B, |u|^2 + |V[pid]|^2
    float* ib; float* io;                                 // [NIp] bias, offset (0 beyond NI)
    float* pm; float* pe; float* psd;                     // [nci][Bp] the chunks' running maximum, sum without the label, label score
    float* rmax; float* cn; float* dcoef; float* rowloss; // [Bp] the row maximum m_i (+inf: a dead row), c_i / tot_i, -c_i A_i, l_i
    float* gpq; float* gpv; float* bpart; int32_t* npart; // [nci][Bp][Dp], [ncs][NIp][Dp] partial gradient tiles; [ncs][NIp] of the bias, of n_j
    float* gu; float* GV; float* Gb;                      // [B][gs] query gradient rows; [NI][D] and [NI]: the dense gradients
    float* partial;                                       // [orx_fullsoftmax_npartials(B)][2] loss / l2 partials of this step
    int* err;
};
struct FullSoftmaxPlan { int64_t Bp, NIp, Dp, tpi, nci, tps, ncs; };
inline int orx_fullsoftmax_npartials(int64_t B) { return (int)((((B + 63) & ~(int64_t)63) + 255) / 256); }
void orx_fullsoftmax_plan(int64_t B, int64_t NI, int32_t D, int32_t chunk_items, int32_t chunk_samples, FullSoftmaxPlan* p);
int orx_launch_fullsoftmax_forward(orx_ctx* ctx, const FullSoftmaxArgs& a);     // prepare, item copy, LSE pass, finalize
int orx_launch_fullsoftmax_grads(orx_ctx* ctx, const FullSoftmaxArgs& a, bool query_side, bool item_side);      // a walk and its finishing pass per side
// what the drivers (below, after the tower's declarations) build a call from: the checks of (B, NI, D, scale, the chunk
// arguments); the scratch of a step as offsets carved behind whatever the form has carved (host_off: a piece for a host
// item_offset); the train mask of a form with the three usual tables
struct FullSoftmaxLayout {
    FullSoftmaxPlan plan; bool host_off;
    size_t xq, xv, key, cw, sq, ib, io, pm, pe, psd, rmax, cn, dcoef, rowloss, off, gpq, gu, gpv, bpart, npart, GV, Gb;
};
int orx_fullsoftmax_check(const char* fn, int64_t B, int64_t NI, int32_t D, float scale, int32_t chunk_items, int32_t chunk_samples);
void orx_fullsoftmax_layout(Carve* cv, int64_t B, int64_t NI, int32_t D, int32_t chunk_items, int32_t chunk_samples, bool grads, bool query_side,
                            bool item_side, bool host_off, FullSoftmaxLayout* l);
int orx_fullsoftmax_mask(const char* fn, orx_table* b, int* train_mask);
int orx_launch_fullsoftmax_lse(orx_ctx* ctx, const FullSoftmaxArgs& a);         // the item copy and the LSE pass alone

// kernels_labelsets.hip (orx_seqrec_full_sets_step / orx_tower_sets_step and their forwards): the full softmax with a label SET
// per sample.  The dense part is the three walks of kernels_fullsoftmax.hip on rows whose key no walked item equals
// (ORX_LS_KEY); the sparse part -- the labels' scores, their sum of item rows, the item side's subtraction -- is here
constexpr int32_t ORX_LS_KEY = 0x7fffffff;                // a live sample's key: above every item of a table of at most 2^31 - 256 rows
struct LabelSetArgs {
    FullSoftmaxArgs fs;                                   // pid unused; key[i] is ORX_LS_KEY or -1
    const int32_t* ptr; const int32_t* items;             // DEVICE [B + 1] offsets, [n] label items
    const float* tw;                                      // DEVICE [n] entry weights (NULL: all ones)
    int64_t n;
    int32_t* owner;                                       // [n] the sample of a list position (-1: no well-formed set covers it)
    float* lp;                                            // [B][D] c_i sum_e t_e V[j_e]; NULL: the forward alone
};
struct LabelSetLayout { size_t ptr, items, tw, owner, lp; };
struct LabelLists { const int32_t* ptr; const int32_t* items; const float* weight; int64_t n; };       // a call's label sets as the caller passed them
// what the SeqRec form and the tower form share (api_fullsoftmax.hip): the checks of the lists before any device work; the
// scratch behind whatever the caller has carved; the lists on the device and the kernels' arguments once d_tmp is grown
// (orx_bag_stage copies host lists); the forward (prepare, item copy, LSE pass, rows, loss partials) and the gradient passes
// (the dense walks, then the labels' part of g_q, the sort of the label entries by item and the item side's runs)
int orx_labelsets_check(const char* fn, const int32_t* lab_ptr, const int32_t* lab_items, int64_t B, int64_t n_lab, bool host);
void orx_labelsets_layout(Carve* cv, int64_t B, int32_t D, int64_t n_lab, bool host, bool host_tw, bool grads, LabelSetLayout* l);
int orx_labelsets_bind(orx_ctx* c, const LabelSetLayout& l, const FullSoftmaxArgs& fs, const int32_t* lab_ptr, const int32_t* lab_items,
                       const float* lab_weight, int64_t n_lab, bool host, bool grads, LabelSetArgs* out);
int orx_launch_labelsets_forward(orx_ctx* ctx, const LabelSetArgs& a);
int orx_launch_labelsets_grads(orx_ctx* ctx, const LabelSetArgs& a, bool query_side, bool item_side);

// kernels_tower.hip (orx_tower_step / orx_tower_loss / orx_tower_query): the dense tower between the pooled history and the full
// softmax's query.  Layer l maps x[l] [B][w[l]] to x[l + 1] [B][w[l + 1]]; every buffer has its own row stride, so that x[L] is
// the full softmax's Q (stride w[L]) and g[L] its gu (stride gs).  Everything but the tables is scratch carved from d_tmp
constexpr int ORX_TOWER_LAYERS = 4, ORX_TOWER_SIDE = 4, ORX_TOWER_WIDTH = 256;
struct TowerArgs {
    int L; int m; int relu_last; int so;                  // layers, side tables, relu on the last layer, so = sum d_j: the pool's first column of x[0]
    int64_t B;
    int w[ORX_TOWER_LAYERS + 1];                          // w[0] = in_0 ... w[L] = the item table's dim
    const float* W[ORX_TOWER_LAYERS]; const float* c[ORX_TOWER_LAYERS];      // [w[l]][w[l + 1]]; [w[l + 1]] or NULL
    float* x[ORX_TOWER_LAYERS + 1]; int ldx[ORX_TOWER_LAYERS + 1];           // activations (all stored: the backward's inputs and relu masks)
    float* g[ORX_TOWER_LAYERS + 1]; int ldg[ORX_TOWER_LAYERS + 1];           // gradients; g[0] NULL: nobody takes it
    float* pw[ORX_TOWER_LAYERS]; float* pc[ORX_TOWER_LAYERS];                // [nch][w[l] w[l + 1]], [nch][w[l + 1]] per-batch-chunk partials; NULL: the tower is not trained
    float* GW[ORX_TOWER_LAYERS]; float* Gc[ORX_TOWER_LAYERS];                // the dense gradients
    int nch; int tpc;                                     // batch chunks of tpc tiles of 64 rows
    float l2x; float l2m;                                 // the coefficient on x[0] (g[0] += l2x x[0]) and on the layers
    const float* S[ORX_TOWER_SIDE]; int64_t srows[ORX_TOWER_SIDE]; int sd[ORX_TOWER_SIDE]; const int32_t* f[ORX_TOWER_SIDE];      // side tables, DEVICE [B] ids
    BagArgs bag;                                          // the history lists (out unused: the pooled row goes to columns [so, w[0]) of x[0])
};
void orx_tower_plan(int64_t B, int* nch, int* tpc);       // a function of B alone
int orx_launch_tower_input(orx_ctx* ctx, const TowerArgs& a);
int orx_launch_tower_forward(orx_ctx* ctx, const TowerArgs& a);                 // one launch per layer
int orx_launch_tower_backward(orx_ctx* ctx, const TowerArgs& a);                // one launch per layer, last to first
int orx_launch_tower_finish(orx_ctx* ctx, const TowerArgs& a);                  // one launch: the partials of all layers in chunk order, + l2m * (W, c)

// ---------------------------------- the host driver of the calls on the softmax over all items (api_fullsoftmax.hip) ---
// A model on this objective is a QUERY FORM: what produces the query matrix Q [NQ][D] and what takes its gradient.  The entry
// point fills one in and calls a driver; the drivers hold everything else once -- the checks of the objective, the lists, the
// scratch of the full softmax and of the label sets, which tables are finished and which stay lazy, the forward and the gradient
// passes (one label per sample, or sets != NULL a label set), the counter, the dense rule on V and b, the losses.
struct FullSoftmaxTable { orx_table* t; bool dense; bool trained; };        // dense: read in full (a layer), so always finished first; else touched by produce
struct FullSoftmaxQuery {                                   // what bind yields
    const float* Q; int64_t NQ; const int32_t* qid;         // the rows the kernels score with; qid arrives as the staged `ids` of the form, if it has any
    const float* X0; int x0w; int x0ld;                     // not NULL: the l2 term sits on these rows and not on the query (FullSoftmaxArgs::l2q = 0)
};
// The drivers call the members in this order, each once per call and `produce` once per step: check, [a step: train], carve, bind,
// then produce, [backward], [apply].  A member may rely on what the earlier ones left in the form (check fills tab[], train sets what
// carve sizes by); a forward never calls train, so the builder leaves every trained / gradient flag false.
struct FullSoftmaxForm {
    const char* fn;
    bool has_ids; const int32_t* ids;                       // a [B] id list of the form's own beside pid (the user table's uid), staged with it
    bool index_flag;                                        // a synchronising step over device lists looks at the index flag at its end
    FullSoftmaxTable tab[1 + ORX_TOWER_SIDE + 2 * ORX_TOWER_LAYERS]; int n_tab;       // the form's tables, in the order they are finished and kept
    bool query_side;                                        // set by train: the gradient passes take the query side
    std::function<int()> check;                             // the form's own checks, before the objective's
    std::function<int(int*)> train;                         // the step's mask: its own bits refused, 0 replaced by every table, tab[].trained and query_side set
    std::function<void(Carve*, bool)> carve;                // its part of d_tmp (grads?)
    std::function<int(bool, FullSoftmaxQuery*)> bind;       // its kernels' arguments once d_tmp is grown; host lists are copied here
    std::function<int(const FullSoftmaxArgs&, bool)> produce;       // per call (step?): touch the rows it reads, launch what writes Q
    std::function<int()> backward;                          // after the gradient passes, before the counter advances (may be empty)
    std::function<int(const FullSoftmaxArgs&)> apply;       // after the counter has advanced: its tables' applies
};
// the kernels' arguments on the context's d_tmp once it is grown, the query's part from q (pid / wt / partial are the drivers' to set)
int orx_fullsoftmax_bind(orx_ctx* c, const FullSoftmaxLayout& l, const FullSoftmaxQuery& q, orx_table* V, orx_table* b, const float* item_offset,
                         int64_t B, float scale, float l2w, FullSoftmaxArgs* out);
int orx_fullsoftmax_drive_step(orx_ctx* c, orx_opt* opt, FullSoftmaxForm& f, orx_table* V, orx_table* b, const int32_t* pid, const LabelLists* sets,
                               const float* weight, const float* item_offset, int64_t B, float scale, float l2_reg, int32_t chunk_items,
                               int32_t chunk_samples, int train_mask, int flags, float* loss_out, float* l2_out);
int orx_fullsoftmax_drive_loss(orx_ctx* c, FullSoftmaxForm& f, orx_table* V, orx_table* b, const int32_t* pid, const LabelLists* sets,
                               const float* weight, const float* item_offset, int64_t B, float scale, int32_t chunk_items, int flags,
                               float* loss_out, float* l2_out, float* row_loss_out);

// kernels_warp.hip (orx_sampler_pairwise_warp): the pairwise draw of `s`, then candidates one after another until one violates the margin
struct WarpNegArgs {
    SamplerArgs s;
    const float* U; const float* V; const float* b;       // b NULL: no item bias
    int model; int D; int T; float margin;
    const float* tw;                                      // DEVICE [T]: the weight of a triplet whose violator is candidate t - 1
    float* weight; int32_t* trials; float* pos_score;     // [n]; trials / pos_score may be NULL
    float* cand_score;                                    // [n * T] or NULL
};
int orx_launch_warpneg(orx_ctx* ctx, const WarpNegArgs& a);

// kernels_vbpr.hip (orx_features_project / orx_vbpr_item_table / orx_vbpr_step / orx_vbpr_loss): VBPR's two products over gathered
// feature rows and the pass over the triplets between them.  Np = Dc rounded up to 16 (registers and LDS only)
struct VbprProjArgs {
    const float* F; const float* E;                       // [NI][Fd] features, [Fd][Dc] projection
    const int32_t* ia; const int32_t* ib;                 // [n] rows (NULL: row0 + k) and the rows subtracted from them (NULL: none)
    int64_t row0; int64_t n; int64_t NI;
    int Fd; int Dc; int Np; int vec;                      // vec: Fd % 4 == 0 and F 16-byte aligned
    float* out; int64_t out_stride; int out_col0;         // out[k * out_stride + out_col0 + c], c < Dc
    int* err;
};
struct VbprPairArgs {
    const float* U; const float* V; const float* b;       // read only; [NU][Dl + Dc], [NI][Dl], [NI] or NULL
    const float* delta;                                   // [B][Dc] (F[p] - F[n]) E
    const int32_t* uid; const int32_t* pid; const int32_t* nid; const float* wt;      // this step's ids [B]; weights or NULL
    float* gu; float* gi; float* R; int32_t* list;        // [B][gs]; [2B][gs], bias gradient in column Dl; [B][Dc] g_k U_c[u_k]; [2B] pid | nid
    int64_t B; int64_t NU; int64_t NI;
    int Dl; int Dc; int gs;
    float invB; float l2w;
    float* partial;                                       // [orx_vbpr_nwaves(ctx, B)][2] loss / l2 partials of this step
    int* err;
};
struct VbprDprojArgs {
    const float* F; const float* R;                       // [NI][Fd]; [B][Dc]
    const int32_t* pid; const int32_t* nid;
    int64_t B; int64_t NI; int64_t chunk_rows;
    int Fd; int Dc; int Np; int vec; int nch;
    float* part;                                          // [nch][Fd][Dc]
    const float* E; float l2p; float* dE;                 // the finishing pass: dE = sum of the partials in chunk order + l2p E
};
int orx_vbpr_nwaves(orx_ctx* ctx, int64_t B);
void orx_vbpr_plan(int64_t B, int32_t Fd, int32_t Dc, int32_t batch_chunk, int32_t out[4]);      // rows per chunk, chunks, padded Dc, tile rows
int orx_launch_vbpr_project(orx_ctx* ctx, const VbprProjArgs& a);
int orx_launch_vbpr_pairs(orx_ctx* ctx, bool grads, const VbprPairArgs& a);
int orx_launch_vbpr_dproj(orx_ctx* ctx, const VbprDprojArgs& a);
int orx_launch_vbpr_copy_cols(orx_ctx* ctx, const float* V, int Dl, float* W, int D, int64_t nrows);      // W[r][0:Dl] = V[r][0:Dl]
