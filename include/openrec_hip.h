/* openrec_hip.h -- C ABI of the MI355X-native OpenRec training hot path.
 *
 * The reference (ylongqi/openrec, /root/reference) has NO FFI boundary: the
 * path is reached through Python classes on top of TensorFlow.  This header is
 * the boundary a maintainer would bind instead (ctypes stub in INTEGRATION.md);
 * every entry point cites the reference interface it replaces (paths relative
 * to /root/reference).
 *
 * Conventions
 *   - every function returns int: 0 = ORX_OK, < 0 = error; the message is
 *     available from orx_last_error() (thread local).  Nothing aborts, no C++
 *     exception crosses the boundary.
 *   - handles (orx_ctx / orx_table / orx_opt) are opaque and owned by the
 *     library; pointer arguments are caller-owned and only need to stay valid
 *     for the duration of the call.
 *   - tables are fp32, row-major [rows, dim], resident in HBM for their whole
 *     life (Keras Embedding weight layout, latent_factor.py:12-15).
 *   - ids are int32 (openrec/tf2/data/dataset.py:113-115).  With
 *     ORX_IDS_DEVICE the id pointers are device pointers, otherwise host.
 *   - calls on one context are serialized on that context's HIP stream; a
 *     context is not thread-safe, distinct contexts are independent.
 *   - there is no CPU fallback: every call fails with ORX_ERR_HIP if no
 *     gfx950 device is usable.
 */
#ifndef OPENREC_HIP_H
#define OPENREC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct orx_ctx orx_ctx;
typedef struct orx_table orx_table;
typedef struct orx_opt orx_opt;

enum orx_status {
    ORX_OK = 0,
    ORX_ERR_ARG = -1,    /* bad argument / handle / shape                      */
    ORX_ERR_HIP = -2,    /* HIP runtime error (message has hipGetErrorString)  */
    ORX_ERR_OOM = -3,    /* device allocation failed                           */
    ORX_ERR_INDEX = -4,  /* id out of range (TF CPU gather raises, bpr.py:23)  */
    ORX_ERR_STATE = -5   /* call sequence error                                */
};

/* tensorflow.keras.optimizers.* used by tf2_examples/bpr_citeulike.py:31.
 * ORX_ADAM is the TF-2.0 sparse rule: EVERY row of a table decays (m, v) and moves (var) at every step.
 * orx_pairwise_step (float4 dims, no censor), orx_dlrm_step and orx_apply_rows apply it lazily: a row takes its
 * gradient-free steps when it is next referenced, and every entry point that observes a table or its slots
 * (read / gather / device_ptr / slot_read / inference / another optimizer / orx_opt_destroy) first brings
 * the rows it exposes up to date, so the result is the dense rule's at every observation.
 * Tables over caller-owned memory (orx_table_wrap) always take the literal whole-table sweeps, as does
 * everything with ORX_ADAM_DENSE=1 in the environment.  A pointer obtained from orx_table_device_ptr is
 * current when returned; after further Adam steps, ask again.
 * ORX_MOMENTUM is keras.optimizers.SGD(lr, momentum > 0, nesterov) (ResourceSparseApplyKerasMomentum /
 * ResourceApplyKerasMomentum): duplicates are summed first, then for each referenced row (every element of a
 * dense variable) with summed gradient G and velocity a (slot 0, zero-initialised)
 *     a = a*momentum - lr*G;   plain: w += a;   nesterov: w += a*momentum - lr*G
 * Rows not referenced in a step are untouched, velocity included.  Momentum takes the exact (non-hogwild) routes of
 * orx_pairwise_step, orx_pointwise_step, orx_apply_rows, orx_dlrm_step and orx_dlrm_dense_apply; ORX_HOGWILD, the
 * sharded engines, orx_shard_grads_sgd and orx_apply_rows_flagged refuse it (ORX_ERR_ARG). */
enum orx_opt_kind { ORX_SGD = 0, ORX_ADAGRAD = 1, ORX_ADAM = 2, ORX_MOMENTUM = 3 };

/* pairwise recommenders: recommenders/bpr.py:5, recommenders/ucml.py:5 */
enum orx_pair_model { ORX_BPR = 0, ORX_UCML = 1 };
/* pointwise recommenders: recommenders/gmf.py:5, recommenders/wrmf.py:5 */
enum orx_point_model { ORX_GMF = 0, ORX_WRMF = 1 };

enum orx_flags {
    ORX_IDS_DEVICE = 1,   /* id / label pointers are device pointers            */
    ORX_HOGWILD = 2,      /* skip duplicate handling: one in-place racy pass
                             (NOT reference semantics; speed comparisons only)  */
    ORX_NO_L2 = 4,        /* objective = loss only (tape over `loss` alone)
                             instead of the example's (loss, l2_loss) tuple     */
    ORX_CENSOR = 8,       /* orx_pairwise_step: after every step, UCML.censor_vec
                             (ucml.py:44-48) on that step's ids: users, then pos
                             items, then neg items, min_norm 0.1                */
    ORX_POINT_SIGMOID = 16, /* orx_pointwise_step / _loss with ORX_WRMF: PointwiseMSELoss(sigmoid=True),
                             the prediction goes through a sigmoid before the weighted squared
                             error (modules/pointwise_mse_loss.py:24-25)        */
    ORX_OUT_DEVICE = 32   /* orx_recommend_topk, orx_score_candidates: the outputs are device pointers */
};

/* kernels whose device time can be sampled with orx_prof_* */
enum orx_kernel_id {
    ORX_K_DEDUP = 0,      /* duplicate-reference detection on the id arrays     */
    ORX_K_FUSED = 1,      /* fused gather-score-loss-grad-update (dominant)     */
    ORX_K_REDUCE = 2,     /* per-step loss reduction (once per call)            */
    ORX_K_SWEEP = 3,      /* Adam dense-decay sweep                             */
    ORX_K_CENSOR = 4,
    ORX_K_POINT = 5,      /* fused pointwise (GMF/WRMF) step                    */
    ORX_K_DUPAPPLY = 6,   /* optimizer apply of the duplicate rows of a step    */
    ORX_K_GEMM = 7,       /* DLRM MLP products (fp32 or fp16 MFMA)              */
    ORX_K_NUM = 8
};

int orx_version(void);
const char* orx_last_error(void);

/* ---- context ----------------------------------------------------------
 * device: HIP ordinal.  stream: an existing hipStream_t to enqueue on (e.g.
 * torch's current stream) or NULL to create a private one. */
int orx_ctx_create(int device, void* stream, orx_ctx** out);
int orx_ctx_destroy(orx_ctx* ctx);
int orx_synchronize(orx_ctx* ctx);
/* Ordering contract for device buffers handed over with ORX_IDS_DEVICE (ids, labels, gradient rows ...): the library
 * reads them on the context's stream.  A buffer produced on ANOTHER stream (a framework's current stream) must be
 * complete there first: orx_ctx_wait_stream makes every later call on `ctx` wait for the work `producer_stream`
 * (a hipStream_t; NULL = the legacy default stream) holds now -- an event, no host synchronisation.  The reference
 * has no such notion: TensorFlow orders its own ops (tf2_examples/bpr_citeulike.py:33-39 runs inside tf.function). */
int orx_ctx_wait_stream(orx_ctx* ctx, void* producer_stream);
/* raises the sticky "id out of range" condition recorded by the kernels
 * (returns ORX_ERR_INDEX once, then clears it).  Synchronizes. */
int orx_check_index_error(orx_ctx* ctx);

/* ---- tables: replace LatentFactor.__init__/variables (latent_factor.py:6-15)
 * orx_table_wrap adopts caller-owned device memory (e.g. a torch tensor). */
int orx_table_create(orx_ctx* ctx, int64_t rows, int32_t dim, orx_table** out);
int orx_table_wrap(orx_ctx* ctx, void* device_ptr, int64_t rows, int32_t dim, orx_table** out);
int orx_table_destroy(orx_table* t);
int64_t orx_table_rows(const orx_table* t);
int32_t orx_table_dim(const orx_table* t);
void* orx_table_device_ptr(const orx_table* t);
/* Keras 'uniform' initializer = U(-0.05, 0.05) / 'zeros' (latent_factor.py:8-11) */
int orx_table_init_uniform(orx_table* t, float lo, float hi, uint64_t seed);
int orx_table_fill(orx_table* t, float value);
/* checkpoint / parity access: rows [row0, row0+nrows) <-> host fp32 */
int orx_table_read(orx_table* t, int64_t row0, int64_t nrows, float* host_dst);
int orx_table_write(orx_table* t, int64_t row0, int64_t nrows, const float* host_src);
/* LatentFactor.__call__ = Embedding gather (bpr.py:23-27): out[k,:] = W[ids[k],:].
 * ids/out are host unless ORX_IDS_DEVICE (then both are device pointers). */
int orx_table_gather(orx_table* t, const int32_t* ids, int64_t n, float* out, int flags);
/* LatentFactor.censor (latent_factor.py:17-23): for each DISTINCT id,
 * W[i] <- W[i] / max(||W[i]||_2, min_norm). */
int orx_table_censor(orx_table* t, const int32_t* ids, int64_t n, float min_norm, int flags);

/* ---- optimizers: replace optimizers.{SGD,Adagrad,Adam}.apply_gradients
 * (tf2_examples/bpr_citeulike.py:31,38) with TF-2.0 sparse-apply semantics.
 *   SGD:     p0..p2 unused
 *   ADAGRAD: p0 = initial_accumulator_value, p1 = epsilon
 *   ADAM:    p0 = beta_1, p1 = beta_2, p2 = epsilon   (dense-decay sparse apply)
 *   MOMENTUM: p0 = momentum in [0, 1], p1 = nesterov (0 or 1), p2 unused */
int orx_opt_create(orx_ctx* ctx, int kind, float lr, float p0, float p1, float p2, orx_opt** out);
int orx_opt_destroy(orx_opt* opt);
int orx_opt_set_lr(orx_opt* opt, float lr);
/* the optimizer's step counter (Keras `optimizer.iterations`: Adam's bias correction depends on it);
 * a checkpoint saves it next to the slots, a resume sets it before the next step.  The step entry points
 * advance it themselves; a host that drives Adam through orx_apply_rows advances it by one per step with
 * orx_opt_advance after the step's gathers and before its applies.
 *   set_step : a jump of the counter (resume, Keras `iterations.assign`).  Every table that is lazily applied
 *              under `opt` is first finished under the old counter; no row is replayed across the jump.
 *   advance  : "the next apply_gradients of `opt` updates exactly these tables" (tf2_examples/bpr_citeulike.py:38 passes
 *              the model's variables): counter += 1.  Keras' Adam touches only the variables it is handed, so any
 *              OTHER table lazily applied under `opt` (a second model sharing the optimizer) is finished first and
 *              takes no decay step for this one.  The step entry points (orx_pairwise_step, orx_pointwise_step,
 *              orx_dlrm_step) do the same for their own tables.  n_tables < 0: the step is over every table the
 *              optimizer holds (an engine with an optimizer of its own): the counter advances, nothing is finished. */
int orx_opt_get_step(orx_opt* opt, int64_t* step_out);
int orx_opt_set_step(orx_opt* opt, int64_t step);
int orx_opt_advance(orx_opt* opt, orx_table* const* tables, int32_t n_tables);
/* read/write an optimizer slot of a table (checkpointing, parity):
 * slot 0 = Adagrad accumulator / Adam m / momentum velocity, slot 1 = Adam v. */
int orx_opt_slot_read(orx_opt* opt, orx_table* t, int slot, int64_t row0, int64_t nrows, float* host_dst);
int orx_opt_slot_write(orx_opt* opt, orx_table* t, int slot, int64_t row0, int64_t nrows, const float* host_src);

/* ---- the hot path ------------------------------------------------------
 * K consecutive train steps of BPR.call / UCML.call + tape.gradient((loss,
 * l2_loss)) + optimizer.apply_gradients  (bpr.py:21-37, ucml.py:21-42,
 * pairwise_log_loss.py:15-34, tf2_examples/bpr_citeulike.py:33-39).
 *   user/item/bias : tables [NU,D], [NI,D], [NI,1].  bias may be NULL with ORX_BPR: BPR without item
 *                    biases (pairwise_log_loss.py:26-30 with p_item_bias = n_item_bias = None, score
 *                    u.p - u.n); ORX_UCML or ORX_CENSOR with a NULL bias returns ORX_ERR_ARG
 *   uid/pid/nid    : int32, step s uses elements [s*id_stride, s*id_stride+B)
 *   margin         : UCML margin (ucml.py:7); ignored for BPR
 *   loss_out/l2_out: host float[K] or NULL (NULL = fully asynchronous call)
 * Gradients of every step are taken on the pre-step tables (snapshot
 * semantics), duplicates handled as TF does (SGD accumulates every
 * occurrence; Adagrad/Adam sum duplicates first). */
int orx_pairwise_step(orx_ctx* ctx, int model, orx_opt* opt,
                      orx_table* user, orx_table* item, orx_table* bias,
                      const int32_t* uid, const int32_t* pid, const int32_t* nid,
                      int64_t K, int64_t B, int64_t id_stride, float margin, int flags,
                      float* loss_out, float* l2_out);

/* The same K steps with a TRAIN MASK: only the tables the mask names receive the steps' updates (Keras updates only the variables
 * handed to apply_gradients, tf2_examples/bpr_citeulike.py:36-38 with a shorter variable list; `layer.trainable = False`).  The
 * use is fold-in -- new users' vectors trained against item tables that are being served --, fine-tuning of one table, and
 * alternating optimisation.  Roles: user, item, bias (ORX_WRMF: the same three).  With T the set of trained roles:
 *   - forward, loss and l2_loss are those of the full step; l2 runs over ALL looked-up rows, trained or not;
 *   - gradients are taken on the pre-step tables (snapshot semantics);
 *   - a table in T receives exactly the update the full step gives it from the same pre-step tables (SGD accumulates every
 *     occurrence; Adagrad, momentum and Adam sum duplicates first; the item table's ids are the positive and negative lookups
 *     concatenated; ORX_NO_L2 drops the l2 part of the gradient);
 *   - a table outside T, and every optimizer slot of it, is bit-for-bit what it was before the call: it is read, never
 *     written.  Slots of a table that was never trained need not exist;
 *   - Adam: the optimizer's counter advances once per step.  A table outside T that is lazily applied under `opt` is finished
 *     under the old counter first and takes no decay for these steps (orx_opt_advance's rule for the model's own frozen tables);
 *   - a K-step call equals K one-step calls; K steps run on the context's stream without host synchronisation, losses are
 *     read once at the end (loss_out = l2_out = NULL: fully asynchronous);
 *   - a mask that names every table the call was given IS orx_pairwise_step / orx_pointwise_step: same route, same bits.
 * ORX_ERR_ARG before any device work: an empty mask; bits outside the three; ORX_TRAIN_BIAS with bias == NULL; and with a
 * strict subset: ORX_HOGWILD, ORX_CENSOR, ORX_GMF (its Dense(1) kernel would be a fourth role).  Ids out of range:
 * ORX_ERR_INDEX as in the full step. */
enum orx_train_mask { ORX_TRAIN_USER = 1, ORX_TRAIN_ITEM = 2, ORX_TRAIN_BIAS = 4 };
int orx_pairwise_step_subset(orx_ctx* ctx, int model, orx_opt* opt,
                             orx_table* user, orx_table* item, orx_table* bias,
                             const int32_t* uid, const int32_t* pid, const int32_t* nid,
                             int64_t K, int64_t B, int64_t id_stride, float margin, int flags,
                             int train_mask, float* loss_out, float* l2_out);

/* Pre-size every per-call scratch buffer for calls of up to K steps of B triplets on these tables
 * (duplicate-detection outputs, rewritten ids, loss partials, scratch tables), so that a later
 * orx_pairwise_step performs no device allocation.  Optional: buffers also grow on demand.
 * bias may be NULL (the tables of a bias-free BPR). */
int orx_pairwise_reserve(orx_ctx* ctx, orx_opt* opt, orx_table* user, orx_table* item, orx_table* bias,
                         int64_t K, int64_t B);

/* Forward only: (loss, l2_loss) of one batch without touching the tables
 * (BPR.call / UCML.call outside a tape).  bias may be NULL as in orx_pairwise_step. */
int orx_pairwise_loss(orx_ctx* ctx, int model,
                      orx_table* user, orx_table* item, orx_table* bias,
                      const int32_t* uid, const int32_t* pid, const int32_t* nid,
                      int64_t B, float margin, int flags, float* loss_out, float* l2_out);

/* The pairwise step with PER-TRIPLET WEIGHTS and an L2 COEFFICIENT: the objective real training runs use.  For step s of the call,
 * with w_i = weight[s*id_stride + i] (1 when weight == NULL):
 *   BPR : loss = (1/B) sum_i w_i * (-log_sigmoid(max(x_i, -30)))     (the weight inside the mean of pairwise_log_loss.py:32)
 *   UCML: loss = sum_i w_i * max(margin - diff_i, 0)                 (inside the sum of ucml.py:39)
 *   J    = loss + l2_reg * l2_loss, l2_loss the model's own term (bpr.py:35, ucml.py:40), never weighted.
 * loss_out[s] is the weighted loss, l2_out[s] the UNSCALED l2_loss (the caller forms J).  A weight of 0 leaves a triplet its l2 part
 * only; weights are not validated (NaN and inf propagate).  weight lives where the ids live (a device pointer under ORX_IDS_DEVICE)
 * and has their stride.  train_mask: as in orx_pairwise_step_subset; 0 = every table the call was given.  Everything else is
 * orx_pairwise_step's contract (snapshot gradients, duplicates per optimizer, lazy Adam, ORX_CENSOR; a K-step call equals K one-step
 * calls; loss_out = l2_out = NULL: fully asynchronous), and weight == NULL with l2_reg == 1 gives its bits.
 * ORX_ERR_ARG before any device work: ORX_HOGWILD (a speed-comparison mode only); l2_reg negative or not finite; ORX_NO_L2 together
 * with l2_reg != 0; and everything orx_pairwise_step / orx_pairwise_step_subset refuse. */
int orx_pairwise_step_weighted(orx_ctx* ctx, int model, orx_opt* opt,
                               orx_table* user, orx_table* item, orx_table* bias,
                               const int32_t* uid, const int32_t* pid, const int32_t* nid, const float* weight,
                               int64_t K, int64_t B, int64_t id_stride, float margin, float l2_reg, int flags,
                               int train_mask, float* loss_out, float* l2_out);

/* Forward only: the weighted loss of orx_pairwise_step_weighted and the unscaled l2_loss of one batch. */
int orx_pairwise_loss_weighted(orx_ctx* ctx, int model,
                               orx_table* user, orx_table* item, orx_table* bias,
                               const int32_t* uid, const int32_t* pid, const int32_t* nid, const float* weight,
                               int64_t B, float margin, int flags, float* loss_out, float* l2_out);

/* ONE POSITIVE AGAINST N NEGATIVES: K train steps of a dot-product model (BPR's tables) under a sampled-softmax or an N-pair
 * log-sigmoid loss.  Sample i of step s has user u = U[uid[s*id_stride + i]], positive p = V[pid[s*id_stride + i]] and negatives
 * n_j = V[nid[(s*id_stride + i)*N + j]], j < N.  Scores are fp32 and of the dot kind only:
 *   s_p = u.p + b[pid],   s_j = u.n_j + b[nid_j] + off_j          (no "+ b" with bias == NULL)
 * off = neg_offset[(s*id_stride + i)*N + j], 0 when neg_offset == NULL: a constant added to a negative's logit -- -log Q(item) when
 * the negatives come from a weighted proposal; -inf removes the negative from the loss.  It is not validated.
 *   ORX_MN_SOFTMAX: l_i = logsumexp(s_p, s_0 .. s_{N-1}) - s_p, evaluated with the maximum subtracted (scores of magnitude 200 give
 *                   finite results); pi_j = exp(s_j - lse)
 *   ORX_MN_LOGSIG : l_i = (1/N) sum_j -log_sigmoid(max(s_p - s_j, -30))      (the clamp of pairwise_log_loss.py:32: N = 1 is BPR's term)
 *   loss    = (1/B) sum_i w_i l_i                  w_i = weight[s*id_stride + i], 1 when weight == NULL
 *   l2_loss = 1/2 (sum |u|^2 + sum |p|^2 + sum over all B*N negatives |n|^2)          no biases (bpr.py:35), never weighted
 *   J       = loss + l2_reg * l2_loss
 * loss_out[s] is the loss, l2_out[s] the UNSCALED l2_loss, as in orx_pairwise_step_weighted.  Gradients, per occurrence and on the
 * pre-step tables, with c_i = w_i / B:
 *   a_ij = c_i pi_j (softmax),   a_ij = c_i sigmoid(s_j - s_p) [s_p - s_j >= -30] / N (logsig),   A_i = sum_j a_ij
 *   g_u = sum_j a_ij n_j - A_i p + l2_reg u,   g_p = -A_i u + l2_reg p,   g_nj = a_ij u + l2_reg n_j,   g_bp = -A_i,   g_bnj = a_ij
 * A_i is the sum of the pi_j themselves (never 1 - pi_p).  Every occurrence is its own term: a negative may repeat inside a sample,
 * may equal the positive, and a row may appear in many samples.  The apply is orx_apply_rows': the user table with the id list
 * uid[B], the item table and the bias with ONE list, pid[B] followed by nid[B*N]; SGD accumulates every occurrence, Adagrad,
 * momentum and Adam sum a row's occurrences over that whole list first, Adam's counter advances once per step.  Lazily-applied
 * Adam: exactly the rows a step reads are brought up to date before it.  A K-step call is K one-step calls; everything runs on the
 * context's stream without a host synchronisation between steps, and loss_out == l2_out == NULL makes the call fully asynchronous.
 * weight and neg_offset live where the ids live (device pointers under ORX_IDS_DEVICE).  No float atomics in the gradient launch
 * or the loss sums: loss_out / l2_out are bit-repeatable, and so are the tables when bias == NULL (the sorted apply).
 * ORX_ERR_ARG before any device work: N outside [1, 64]; an unknown loss kind; ORX_HOGWILD or ORX_CENSOR; l2_reg negative or not
 * finite; ORX_NO_L2 with l2_reg != 0; user dim != item dim; a bias that is not [item rows, 1]; tables or optimizer on another
 * context; what orx_apply_rows refuses for the optimizer and the tables (ORX_ADAM_DENSE with a bias).  Not offered: train masks,
 * UCML / L2 scoring, the sharded engines.  An id outside its table: ORX_ERR_INDEX as orx_pairwise_step reports it (the gradient
 * launch checks every id and never uses a bad one as an address: such a user or positive zeroes its sample, such a negative
 * itself); the context stays usable.  K == 0 or B == 0: ORX_OK, nothing is launched. */
enum orx_multineg_kind { ORX_MN_SOFTMAX = 0, ORX_MN_LOGSIG = 1 };
int orx_multineg_step(orx_ctx* ctx, int loss_kind, orx_opt* opt,
                      orx_table* user, orx_table* item, orx_table* bias /* NULL ok */,
                      const int32_t* uid, const int32_t* pid, const int32_t* nid,
                      const float* weight /* NULL ok */, const float* neg_offset /* NULL ok */,
                      int64_t K, int64_t B, int32_t N, int64_t id_stride, float l2_reg, int flags,
                      float* loss_out, float* l2_out);
/* Forward only: (loss, l2_loss) of one batch of orx_multineg_step, by the loss-only form of its kernel: no gradient is written, no
 * table changes.  On the same tables it gives the step's loss_out / l2_out bit for bit.  flags: ORX_IDS_DEVICE. */
int orx_multineg_loss(orx_ctx* ctx, int loss_kind,
                      orx_table* user, orx_table* item, orx_table* bias /* NULL ok */,
                      const int32_t* uid, const int32_t* pid, const int32_t* nid,
                      const float* weight /* NULL ok */, const float* neg_offset /* NULL ok */,
                      int64_t B, int32_t N, int flags, float* loss_out, float* l2_out);

/* IN-BATCH NEGATIVES: K train steps of a dot-product model (BPR's tables) under the full-batch softmax of retrieval / two-tower
 * training (Yi et al. 2019): the positive of every sample is scored against the positives of ALL samples of the batch.  No B x B
 * matrix is stored.  Step s has B samples (uid[s*id_stride + i], pid[s*id_stride + i]); the item bias table is optional.
 *   u_i = U[uid[i]],  v_j = V[pid[j]],  b_j = b[pid[j]]   (0 with bias == NULL)
 *   s_ij = scale * (u_i . v_j + b_j) + off_j
 * scale is finite and > 0 (1 / temperature).  off = item_offset[s*id_stride + j], 0 when item_offset == NULL: added to column j in
 * every row, the diagonal included -- typically -log Q(pid[j]).  It must be finite and is not validated.
 * Hit masking: hit(i, j) is true when ORX_IB_MASK_HITS is set, j != i and pid[j] == pid[i] (the row's own positive is not a
 * negative).  N(i) = { j : not hit(i, j) } is the set of columns of row i, so i is always in N(i).
 *   lse_i = logsumexp over j in N(i) of s_ij      evaluated with the maximum subtracted: |s| of 200 gives finite results
 *   l_i   = lse_i - s_ii                          = log1p(sum over j != i of exp(s_ij - s_ii)) when the diagonal holds the maximum
 *   loss    = (1/B) sum_i w_i l_i                 w_i = weight[s*id_stride + i], 1 when weight == NULL
 *   l2_loss = 1/2 (sum_i |u_i|^2 + sum_i |v_i|^2) over the 2B looked-up rows: no biases, never weighted
 *   J       = loss + l2_reg * l2_loss
 * loss_out[s] is the loss, l2_out[s] the UNSCALED l2_loss, as in orx_multineg_step.  Gradients, per occurrence and on the pre-step
 * tables, with c_i = w_i / B:
 *   pi_ij = exp(s_ij - lse_i) for j in N(i), else 0;   A_i = sum over j != i of pi_ij  (the pi themselves, never 1 - pi_ii)
 *   a_ij  = c_i pi_ij (j != i),   a_ii = -c_i A_i
 *   g_u[i] = scale * sum_j a_ij v_j + l2_reg u_i,   g_v[j] = scale * sum_i a_ij u_i + l2_reg v_j,   g_b[j] = scale * sum_i a_ij
 * The apply is orx_apply_rows': the user table with uid[B], then the item table and the bias with pid[B]; SGD accumulates every
 * occurrence, Adagrad, momentum and Adam sum a row's occurrences first, Adam's counter advances once per step.  Lazily-applied
 * Adam: exactly the rows a step reads are brought up to date before it.  A K-step call is K one-step calls, bit for bit;
 * everything runs on the context's stream without a host synchronisation between steps, and loss_out == l2_out == NULL makes the
 * call fully asynchronous.  weight and item_offset live where the ids live.  No float atomics in the step's own kernels or the
 * loss sums: loss_out, l2_out and the row losses are bit-repeatable, and so are the tables when bias == NULL (the sorted apply).
 * chunk_cols: 0 -- the launcher splits the columns of a row block into chunks as it sees fit, from (B, D) alone --, or a multiple
 * of the tile width 64: that many columns per chunk.  flags: ORX_IDS_DEVICE, ORX_NO_L2, ORX_IB_MASK_HITS.
 * B == 1: l = 0, only the l2 gradient moves the rows.  K == 0 or B == 0: ORX_OK, nothing is launched.
 * ORX_ERR_ARG before any device work: scale not finite or <= 0; l2_reg negative or not finite; ORX_NO_L2 with l2_reg != 0;
 * ORX_HOGWILD or ORX_CENSOR; user dim != item dim, or a dim above 256; a bias that is not [item rows, 1]; tables or optimizer on
 * another context; chunk_cols negative or no multiple of 64; what orx_apply_rows refuses (ORX_ADAM_DENSE with a bias).
 * An id outside its table: ORX_ERR_INDEX as orx_multineg_step reports it.  The bad id is never used as an address; its sample
 * contributes no loss, no l2 and no gradient and leaves every other row's softmax as a column; the context stays usable.
 * Not offered: UCML / L2 scoring, train masks, the sharded engines, a symmetric (item -> user) loss. */
enum orx_inbatch_flags { ORX_IB_MASK_HITS = 0x1000 };
int orx_inbatch_step(orx_ctx* ctx, orx_opt* opt,
                     orx_table* user, orx_table* item, orx_table* bias /* NULL ok */,
                     const int32_t* uid, const int32_t* pid,
                     const float* weight /* NULL ok */, const float* item_offset /* NULL ok */,
                     int64_t K, int64_t B, int64_t id_stride, float scale, float l2_reg, int32_t chunk_cols, int flags,
                     float* loss_out, float* l2_out);
/* Forward only, by the same kernels: (loss, l2_loss) of one batch -- the step's loss_out / l2_out bit for bit on the same tables
 * -- and, if row_loss_out is not NULL, l_i of every sample ([B], where the ids live; 0 for a sample with an id out of range).
 * No table changes.  flags: ORX_IDS_DEVICE, ORX_IB_MASK_HITS. */
int orx_inbatch_loss(orx_ctx* ctx,
                     orx_table* user, orx_table* item, orx_table* bias /* NULL ok */,
                     const int32_t* uid, const int32_t* pid,
                     const float* weight /* NULL ok */, const float* item_offset /* NULL ok */,
                     int64_t B, float scale, int32_t chunk_cols, int flags,
                     float* loss_out, float* l2_out, float* row_loss_out /* NULL ok */);
/* What the launcher does for (B, D, chunk_cols): out = { own rows per workgroup, columns per tile, column chunks per row block,
 * padded dim }.  No device is needed. */
int orx_inbatch_geometry(int64_t B, int32_t D, int32_t chunk_cols, int32_t out[4]);

/* K train steps of GMF.call / WRMF.call (gmf.py:22-34, wrmf.py:21-34,
 * pointwise_mse_loss.py:18-31).  w: GMF's Dense(1, use_bias=False) kernel as a
 * [D,1] table (NULL for WRMF).  a, b: WRMF confidence weights (wrmf.py:7). */
int orx_pointwise_step(orx_ctx* ctx, int model, orx_opt* opt,
                       orx_table* user, orx_table* item, orx_table* bias, orx_table* w,
                       const int32_t* uid, const int32_t* iid, const float* label,
                       int64_t K, int64_t B, int64_t id_stride, float a, float b, int flags,
                       float* loss_out, float* l2_out);

/* orx_pointwise_step with a train mask (see orx_pairwise_step_subset): ORX_WRMF, with or without ORX_POINT_SIGMOID. */
int orx_pointwise_step_subset(orx_ctx* ctx, int model, orx_opt* opt,
                              orx_table* user, orx_table* item, orx_table* bias, orx_table* w,
                              const int32_t* uid, const int32_t* iid, const float* label,
                              int64_t K, int64_t B, int64_t id_stride, float a, float b, int flags,
                              int train_mask, float* loss_out, float* l2_out);

/* orx_pointwise_step / orx_pointwise_step_subset with the objective J = loss + l2_reg * l2_loss (gmf.py:32 -- the Dense kernel
 * included --, wrmf.py:32); l2_out stays the unscaled l2_loss.  No sample weights here: WRMF has a and b.  train_mask 0: every
 * table.  ORX_ERR_ARG before any device work: ORX_HOGWILD, l2_reg negative or not finite, ORX_NO_L2 with l2_reg != 0, and what the
 * two plain entry points refuse.  l2_reg == 1 gives orx_pointwise_step's bits. */
int orx_pointwise_step_l2reg(orx_ctx* ctx, int model, orx_opt* opt,
                             orx_table* user, orx_table* item, orx_table* bias, orx_table* w,
                             const int32_t* uid, const int32_t* iid, const float* label,
                             int64_t K, int64_t B, int64_t id_stride, float a, float b, float l2_reg, int flags,
                             int train_mask, float* loss_out, float* l2_out);

/* Forward only for the pointwise models (GMF.call / WRMF.call outside a tape). */
int orx_pointwise_loss(orx_ctx* ctx, int model,
                       orx_table* user, orx_table* item, orx_table* bias, orx_table* w,
                       const int32_t* uid, const int32_t* iid, const float* label,
                       int64_t B, float a, float b, int flags, float* loss_out, float* l2_out);

/* Recommender.inference (bpr.py:39-43, wrmf.py:36-40: kind 0 = U[uid] . V^T + b;
 * ucml.py:50-53: kind 1 = -||U[uid] - V||^2 + b; gmf.py:36-41: kind 2 = sum_d w_d u_d v_d + b).
 * uid: host int32[n]; out: host float[n * item_rows], row-major [n, item_rows].
 * bias may be NULL (every kind): the same scores without the "+ b" (a model without item biases). */
int orx_score_all_items(orx_ctx* ctx, int kind, orx_table* user, orx_table* item, orx_table* bias, orx_table* w,
                        const int32_t* uid, int64_t n, float* out);

/* orx_score_all_items with the scores left on the device: out_dev device float[n * item_rows]. */
int orx_score_all_items_device(orx_ctx* ctx, int kind, orx_table* user, orx_table* item, orx_table* bias, orx_table* w,
                               const int32_t* uid, int64_t n, float* out_dev);

/* Ranking metrics of the evaluation step (openrec/tf2/metrics/ranking_metrics.py:8-69; eval_step in
 * tf2_examples/bpr_citeulike.py:41-46).  For each of n users: scores over ALL items (computed on the
 * device like orx_score_all_items when pred == NULL, else taken from the host array pred[n*items]),
 * pos_mask / excl_mask host uint8 [n*items]; at: host float[nat] cut-offs (nat <= 16).
 * Outputs (host): auc[n], ndcg[n*nat], recall[n*nat]; any of them may be NULL.  bias may be NULL as in
 * orx_score_all_items. */
int orx_rank_metrics(orx_ctx* ctx, int kind, orx_table* user, orx_table* item, orx_table* bias, orx_table* w,
                     const int32_t* uid, const float* pred, const uint8_t* pos_mask, const uint8_t* excl_mask,
                     int64_t n, int64_t items, const float* at, int32_t nat,
                     float* auc, float* ndcg, float* recall);

/* The same metrics with the two masks as CSR item lists over the call's n users (the form the reference's Dataset holds them
 * in before openrec/tf2/data/dataset.py:60-82 _evaluation_generator densifies them): pos_ptr / excl_ptr host int64[n + 1]
 * starting at 0, pos_items / excl_items host int32, each user's list a set (a repeated positive is an error, an id outside
 * [0, items) an index error).  2 x n x items mask bytes become the lists; results equal orx_rank_metrics on the dense masks.
 * pred_on_device != 0: pred is device memory (what orx_score_all_items_device wrote).  bias may be NULL as in orx_score_all_items. */
int orx_rank_metrics_csr(orx_ctx* ctx, int kind, orx_table* user, orx_table* item, orx_table* bias, orx_table* w,
                         const int32_t* uid, const float* pred, int32_t pred_on_device, int64_t n, int64_t items,
                         const int64_t* pos_ptr, const int32_t* pos_items, const int64_t* excl_ptr, const int32_t* excl_items,
                         const float* at, int32_t nat, float* auc, float* ndcg, float* recall);

/* orx_rank_metrics_csr with pred == NULL, without the [n, item_rows] score matrix or any other buffer of that size: kinds,
 * bias == NULL, w, at / nat, outputs and error codes as there, results equal to it bit for bit.
 *   lists      each user's pos_items and excl_items rows must be STRICTLY ASCENDING (what SparseMask.from_lists / from_dense
 *              produce); anything else is ORX_ERR_ARG naming the user.  An id outside [0, item rows) or a uid outside
 *              [0, user rows) is ORX_ERR_INDEX.  All of this is checked on the host before any launch.
 *   scratch    users are processed in batches so that the device scratch made for the call stays within scratch_bytes
 *              (0: 512 MB).  dot / GMF with dim <= 128: per user the two lists with their scores and 3 x 64 words of
 *              thresholds and counters.  L2, dim > 128 and ORX_SCORE_SIMPLE: the scorer itself into a bounded piece of score
 *              rows plus the sweeps of orx_rank_metrics_csr.  When not even the smallest batch fits (one user; its score rows
 *              are 65 when n > 64 on the dense route, the scorer's 128-user tile) the call exceeds the budget for that one
 *              batch; orx_rank_metrics_matrixfree_scratch tells beforehand.
 * Lazy tables are synced first.  A repeated call gives the same bits. */
int orx_rank_metrics_matrixfree(orx_ctx* ctx, int kind, orx_table* user, orx_table* item, orx_table* bias, orx_table* w,
                                const int32_t* uid, int64_t n,
                                const int64_t* pos_ptr, const int32_t* pos_items,
                                const int64_t* excl_ptr, const int32_t* excl_items,
                                const float* at, int32_t nat, size_t scratch_bytes,
                                float* auc, float* ndcg, float* recall);

/* Host only: the device scratch (*bytes) and the users per batch orx_rank_metrics_matrixfree would use for n users, `items`
 * item rows of dimension dim, lists of at most max_pos / max_excl items per user and the given budget (0: the default).  The
 * entry point sizes its buffers with this function. */
int orx_rank_metrics_matrixfree_scratch(int64_t n, int64_t items, int32_t dim, int32_t kind, int64_t max_pos, int64_t max_excl,
                                        size_t scratch_bytes, int64_t* bytes, int64_t* users_per_batch);

/* Host only: the list checks orx_rank_metrics_matrixfree makes before any launch (offsets from 0 that never decrease, ids
 * inside [0, items) else ORX_ERR_INDEX, every row strictly ascending else ORX_ERR_ARG naming the user); the longest lists out. */
int orx_rank_metrics_matrixfree_check(int64_t n, int64_t items, const int64_t* pos_ptr, const int32_t* pos_items,
                                      const int64_t* excl_ptr, const int32_t* excl_items, int64_t* max_pos, int64_t* max_excl);

/* ---- candidate lists (beyond the reference API: the re-ranking stage after orx_recommend_topk or any external retrieval, and
 * the evaluation against sampled or explicit negatives of openrec/tf2/data/dataset.py:70-74 without masks over all items).
 * Kinds, bias == NULL and w as in orx_score_all_items; uid host int32[n]; cand_ptr host int64[n + 1] from 0, cand_items host
 * int32: the items listed for each user.  The work and the device scratch grow with the listed entries, not with
 * n x item rows.  An item id outside [0, item rows) or a uid outside [0, user rows) is ORX_ERR_INDEX, found on the host before
 * any launch (the context stays usable).  Lazy tables are synced first.  A repeated call gives the same bits; the result does
 * not depend on launch shapes or atomics.
 *   dot / GMF with dim <= 128: the listed item rows are gathered through the matrix cores with the scorer's operand layout and
 *   k order.  L2, dim > 128 and ORX_SCORE_SIMPLE: the scorer itself writes the score rows of a bounded batch of users and the
 *   listed entries are picked out of them (no faster in compute; the masks over all items are still gone).
 *
 * orx_score_candidates: out[e] = the score of entry e, bit for bit the element [q, cand_items[e]] that orx_score_all_items
 * writes for that user.  A list may be in any order and may repeat items.  out: float[cand_ptr[n]], host memory, device memory
 * with flags = ORX_OUT_DEVICE. */
int orx_score_candidates(orx_ctx* ctx, int kind, orx_table* user, orx_table* item, orx_table* bias, orx_table* w,
                         const int32_t* uid, int64_t n, const int64_t* cand_ptr, const int32_t* cand_items, int flags, float* out);

/* The ranking metrics of each user over the universe cand[q]: bit for bit (NaN-aware) what orx_rank_metrics_csr returns for the
 * same pos lists and the exclusion lists [0, item rows) \ cand[q] -- AUC over cand \ pos against every positive, a positive
 * outside cand ranked as an excluded positive, 0 / 0 -> NaN.  Every row of both lists must be STRICTLY ASCENDING, anything else
 * is ORX_ERR_ARG naming the user and the list.  at / nat (<= 16) and the outputs (any may be NULL) as in orx_rank_metrics_csr.
 * Users are processed in batches so that the device scratch of a call (the lists, their scores, on the dense route the piece
 * of score rows) stays within scratch_bytes (0: 512 MB); a single user whose own lists exceed it runs as a batch of one. */
int orx_rank_metrics_candidates(orx_ctx* ctx, int kind, orx_table* user, orx_table* item, orx_table* bias, orx_table* w,
                                const int32_t* uid, int64_t n,
                                const int64_t* pos_ptr, const int32_t* pos_items,
                                const int64_t* cand_ptr, const int32_t* cand_items,
                                const float* at, int32_t nat, size_t scratch_bytes,
                                float* auc, float* ndcg, float* recall);

/* Host only: the list checks orx_rank_metrics_candidates makes before any launch (offsets from 0 that never decrease, ids
 * inside [0, items) else ORX_ERR_INDEX, every row strictly ascending else ORX_ERR_ARG naming the user and the list); the
 * longest lists out. */
int orx_rank_metrics_candidates_check(int64_t n, int64_t items, const int64_t* pos_ptr, const int32_t* pos_items,
                                      const int64_t* cand_ptr, const int32_t* cand_items, int64_t* max_pos, int64_t* max_cand);

/* ---- top-K recommendation (beyond the reference API: what `Recommender.inference` is used for after training).
 * For each user q of uid[n] (host int32) the k items with the largest orx_score_all_items score s(q, j) -- the same kinds,
 * bias may be NULL, w for GMF -- without materialising the [n, item_rows] score matrix.
 *   order     score descending, then item id ascending (tf.math.top_k's tie rule)
 *   scores    bit-identical to orx_score_all_items for that (q, j)
 *   eligible  not in the user's exclusion list and not NaN (-inf is an ordinary score); fewer than k eligible items leave
 *             the rest of the row as item -1, score -inf
 *   excl_ptr  host int64[n + 1] from 0 and excl_items host int32: each user's excluded items (the orx_rank_metrics_csr
 *             form; either may be NULL for none)
 * 1 <= k <= 1024 (else ORX_ERR_ARG); a uid outside [0, user rows) or an excluded id outside [0, item rows) is ORX_ERR_INDEX.
 * Outputs out_items int32[n * k], out_scores float[n * k]: host memory, device memory with flags = ORX_OUT_DEVICE.
 * The result does not depend on launch shapes or atomics: a repeated call gives the same bits.  Lazy tables are synced. */
int orx_recommend_topk(orx_ctx* ctx, int kind, orx_table* user, orx_table* item, orx_table* bias, orx_table* w,
                       const int32_t* uid, int64_t n, const int64_t* excl_ptr, const int32_t* excl_items, int32_t k, int flags,
                       int32_t* out_items, float* out_scores);

/* The same selection and rules over scores that exist already: scores float[n * m] row-major, in device memory when
 * scores_on_device != 0 (e.g. what orx_score_all_items_device wrote), else on the host.  excl_ptr / excl_items as in
 * orx_recommend_topk with ids in [0, m); outputs on the host. */
int orx_topk_rows(orx_ctx* ctx, const float* scores, int32_t scores_on_device, int64_t n, int64_t m,
                  const int64_t* excl_ptr, const int32_t* excl_items, int32_t k, int32_t* out_items, float* out_scores);

/* ---- on-device triplet sampler: the producer of the train step
 * (openrec/tf2/data/dataset.py:7-16 _pairwise_generator; utils.py:82-87, 102-116).
 * rec_user / rec_item: the n_records interaction records; csr_ptr[total_users + 1] / csr_items: the
 * positives of every user, item ids sorted ascending inside a row (host arrays, copied to the device).
 * orx_sampler_pairwise writes samples [first, first + n) of the stream `seed` to DEVICE arrays:
 * every record is the positive exactly once per epoch of n_records samples (keyed permutation);
 * negatives are uniform over the items that are not positives of the user.  Sample g depends only
 * on (seed, g), never on the launch shape. */
typedef struct orx_sampler orx_sampler;
int orx_sampler_create(orx_ctx* ctx, const int32_t* rec_user, const int32_t* rec_item, int64_t n_records,
                       const int64_t* csr_ptr, const int32_t* csr_items, int64_t total_users, int64_t total_items,
                       orx_sampler** out);
int orx_sampler_destroy(orx_sampler* s);
int orx_sampler_pairwise(orx_sampler* s, uint64_t seed, int64_t first, int64_t n,
                         int32_t* uid_dev, int32_t* pid_dev, int32_t* nid_dev);
/* Dynamic negative sampling: (user, positive) of samples [first, first + n) exactly as orx_sampler_pairwise gives them, and as
 * the negative the HARDEST of n_cand uniform candidates: the one the current model scores highest.  Candidate c of sample g is a
 * uniform item that is not a positive of the user; it depends on (seed, g, c) only (never on n_cand, n, first or the launch
 * shape), and candidate 0 is the negative of orx_sampler_pairwise, so n_cand = 1 is that call bit for bit.  Candidates of a
 * sample are independent and may repeat.  Scores are fp32 of the kinds of orx_score_all_items: ORX_BPR U[u].V[c] + b[c],
 * ORX_UCML -||U[u] - V[c]||^2 + b[c]; bias may be NULL (no "+ b").  nid is the candidate with the largest score; equal scores:
 * the smallest c; a NaN score never wins against a number; all NaN: candidate 0.  No atomics: a repeated call gives the same bits.
 * cand_dev / cand_score_dev (DEVICE, [n * n_cand] row-major, or NULL): every candidate and the score the selection saw.
 * ORX_ERR_ARG before any launch: n_cand outside [1, 64], a model other than BPR / UCML, tables on another context than the
 * sampler's, user rows != total_users, item rows != total_items, user dim != item dim, a bias that is not [total_items, 1].
 * n = 0: ORX_OK, nothing is launched.  Lazily-applied Adam: the rows read are drawn on the device, so the WHOLE of user, item and
 * bias is brought up to date first (as orx_score_all_items does), not only the exposed rows; the next Adam step makes the tables
 * lazy again.  Runs on the context's stream, no host synchronisation. */
int orx_sampler_pairwise_hard(orx_sampler* s, int model, orx_table* user, orx_table* item, orx_table* bias,
                              uint64_t seed, int64_t first, int64_t n, int32_t n_cand,
                              int32_t* uid_dev, int32_t* pid_dev, int32_t* nid_dev,
                              int32_t* cand_dev /* [n*n_cand] or NULL */, float* cand_score_dev /* [n*n_cand] or NULL */);
/* The negatives of orx_multineg_step: (user, positive) of samples [first, first + n) exactly as orx_sampler_pairwise gives them,
 * and nid_dev[i * n_neg + j] = candidate j of sample first + i of orx_sampler_pairwise_hard, bit for bit, with or without a
 * proposal -- the draws alone, no table is read and nothing is scored.  n_neg = 1 is orx_sampler_pairwise.  A window does not
 * depend on how it is split into calls.  ORX_ERR_ARG before any launch: n_neg outside [1, 64], a NULL output with n > 0.
 * n = 0: ORX_OK, nothing is launched.  Runs on the context's stream, no host synchronisation. */
int orx_sampler_pairwise_multi(orx_sampler* s, uint64_t seed, int64_t first, int64_t n, int32_t n_neg,
                               int32_t* uid_dev, int32_t* pid_dev, int32_t* nid_dev /* [n * n_neg] */);
/* WARP negatives: (user, positive) of samples [first, first + n) exactly as orx_sampler_pairwise gives them, and as the negative
 * the FIRST of up to T = max_trials candidates that violates the margin against the positive under the current model; the
 * triplet's weight is trial_weight[number of candidates it took - 1], a function of WARP's rank estimate
 * floor((items - 1) / trials) that the caller tabulates (host array [T]: any rank loss, exact bits, no transcendental on the device).
 * Stream: candidate c of sample g is candidate c of orx_sampler_pairwise_hard -- the same seed_c, rejection loop and 256-attempt
 * limit, from the proposal when one is set (orx_sampler_set_proposal) -- so candidate 0 is the pairwise negative.
 * Scores: fp32, the kinds of orx_sampler_pairwise_hard (ORX_BPR U[u].V[j] + b[j], ORX_UCML -||U[u] - V[j]||^2 + b[j]; bias may be
 * NULL: no "+ b"), s_p for the positive and s_c for candidate c, by one scorer.  Summation order: the products of four adjacent
 * columns as (x0 + x1) + (x2 + x3), those partial sums by a butterfly over the columns' lanes (xor 1, 2, 4, ...), the bias last; a
 * dim that is no multiple of 4 or above 256: columns l, l + 64, .. in order per lane l, the butterfly over 64 lanes, the bias.  The
 * scores are this kernel's own: bit equality with cand_score of orx_sampler_pairwise_hard is NOT promised (two kernels).
 * Violation: candidate c violates iff (s_c + margin) > s_p -- one rounded fp32 add, then a compare; a NaN on either side never
 * violates; margin may be +inf or -inf.  For ORX_UCML this is "the hinge max(margin - (s_p - s_c), 0) of the
 * reference's UCML (recommenders/ucml.py:39) is active for (u, p, c)".
 * Result: t = 1 + the smallest violating c < T, or 0 when none of the T candidates violates.
 *   nid[i]        = candidate t - 1, or candidate 0 when t = 0
 *   weight[i]     = trial_weight[t - 1], or exactly +0.0f when t = 0 (orx_pairwise_step_weighted: such a triplet keeps only its l2 part)
 *   trials[i]     = t                                                            (trials_dev [n] or NULL)
 *   pos_score[i]  = s_p                                                          (pos_score_dev [n] or NULL)
 *   cand_score[i * T + c] = s_c for every c < t, or every c < T when t = 0       (cand_score_dev [n * T] or NULL)
 * and cand_score entries beyond that are unspecified (the kernel may or may not have scored them, and writes none it did not scan).
 * Independence: a sample's outputs depend on (seed, g), the tables, margin and trial_weight only -- never on n, first, the launch
 * shape or how candidates are grouped into rounds.  No atomics: a repeated call gives the same bits.
 * Prefix rule: for T1 < T2 a sample with t(T1) > 0 has t(T2) = t(T1) and the same nid; one with t(T1) = 0 has t(T2) = 0 or
 * T1 < t(T2) <= T2.
 * Weight table: kept on the device inside the sampler and uploaded only when its T floats differ (as bits) from the copy already
 * there, so a loop that passes the same table enqueues the call without a host synchronisation; a CHANGED table may synchronise
 * the context's stream, as orx_sampler_set_proposal does.
 * ORX_ERR_ARG before any launch: everything orx_sampler_pairwise_hard refuses, max_trials outside [1, 256], a NaN margin,
 * trial_weight == NULL, weight_dev == NULL with n > 0.  n = 0: ORX_OK, nothing is launched.  Lazily-applied Adam: the WHOLE of
 * user, item and bias is brought up to date first, as in orx_sampler_pairwise_hard.  Runs on the context's stream. */
int orx_sampler_pairwise_warp(orx_sampler* s, int model, orx_table* user, orx_table* item, orx_table* bias,
                              uint64_t seed, int64_t first, int64_t n, int32_t max_trials, float margin,
                              const float* trial_weight /* HOST [max_trials] */,
                              int32_t* uid_dev, int32_t* pid_dev, int32_t* nid_dev, float* weight_dev,
                              int32_t* trials_dev      /* [n] or NULL */,
                              float* pos_score_dev     /* [n] or NULL */,
                              float* cand_score_dev    /* [n * max_trials] or NULL */);
/* ---- negatives from a weighted item proposal (popularity^alpha, in-stock items, ...).
 * orx_alias_build: host only, no context or device: the Walker / Vose alias table of n weights, computed in double.  Column j
 * holds a 32-bit threshold thr[j] and an alias alias[j]: with a uniform 32-bit t, column j yields j if t < thr[j] and alias[j]
 * otherwise, so a uniform column and a uniform t draw item i with probability w[i] / sum(w) up to the 32-bit quantisation.
 * A column that keeps all of its mass has alias[j] == j (its threshold is then irrelevant).  An item of weight 0 is never an
 * outcome: its own column has thr == 0 and no column aliases to it, the columns rounding leaves over at the end of Vose's
 * loop included.  ORX_ERR_ARG, nothing written: n < 1, n > INT32_MAX, a NaN, infinite or negative weight, all weights 0.
 *
 * orx_sampler_set_proposal: weights is a HOST array [total_items], or NULL for uniform negatives again.  The table of
 * orx_alias_build is kept on the device, one 8-byte record (thr, alias) per item.  The call may synchronise the context's
 * stream: draws enqueued before it see the old table, draws after it the new one.  Bad weights: ORX_ERR_ARG, and the proposal
 * that was in force stays in force.  orx_sampler_proposal_read copies the device table back into host arrays [total_items];
 * ORX_ERR_ARG when no proposal is set.
 *
 * With a proposal set, attempt a of candidate c of sample g of orx_sampler_pairwise (c = 0) / orx_sampler_pairwise_hard is
 *     r    = mix64(seed_c ^ (g * 0x9E3779B97F4A7C15) ^ (a << 56) ^ 0xA5A5A5A5)      the word the uniform draw forms
 *     j    = r % total_items
 *     t    = (uint32)(mix64(r ^ 0x5851F42D4C957F2D) >> 32)
 *     item = t < thr[j] ? j : alias[j]
 * re-drawn while item is a positive of the user (at most 256 attempts, then the last draw is kept, as without a proposal).
 * Everything else of the two streams is unchanged: (u, p), candidate 0 = the pairwise negative, dependence on (seed, g, c)
 * only, no atomics.  Without a proposal both calls give the bits they always gave; with all weights equal to 1.0 every column
 * keeps its mass and the stream is the uniform one bit for bit.  The pointwise producers below draw uniform negatives only:
 * they return ORX_ERR_ARG before any launch while a proposal is set. */
int orx_alias_build(const double* weights, int64_t n, uint32_t* thr_out, int32_t* alias_out);
int orx_sampler_set_proposal(orx_sampler* s, const double* weights /* host [total_items], or NULL = uniform again */);
int orx_sampler_proposal_read(orx_sampler* s, uint32_t* thr_out, int32_t* alias_out);

/* Per-record weights for orx_pairwise_step_weighted, delivered on the device.  orx_sampler_set_record_weights: host_w is a HOST
 * array [n_records] in the order of the records given to orx_sampler_create (copied to the device; not validated), or NULL to drop
 * them.  orx_sampler_pairwise_weights: w_dev[i] (a DEVICE array [n]) = the weight of the record that sample first + i of stream
 * `seed` draws as its positive -- the keyed permutation of orx_sampler_pairwise / orx_sampler_pairwise_hard, with or without a
 * proposal; it depends on (seed, first + i) only.  ORX_ERR_STATE while no record weights are set; n = 0: ORX_OK, no launch. */
int orx_sampler_set_record_weights(orx_sampler* s, const float* host_w /* [n_records] or NULL */);
int orx_sampler_pairwise_weights(orx_sampler* s, uint64_t seed, int64_t first, int64_t n, float* w_dev);
/* The pointwise producers of GMF / WRMF (dataset.py:18-36 _stratified_pointwise_generator, :38-58
 * _per_pos_stratified_pointwise_generator): samples [first, first + n) as (user, item, label) DEVICE arrays.
 *   stratified         : with probability pos_ratio the next record of the shuffled epoch (label 1), otherwise a uniform
 *                        (user, item) pair that is not a positive (label 0).  Sequential stream, like the reference's
 *                        generator: a call continues at the sample the previous one (same seed) stopped at; first = 0 restarts.
 *   per_pos_stratified : groups of 1 + int((1 - pos_ratio) / pos_ratio): a record (label 1), then that many DISTINCT items
 *                        other than the record's (label 0; not checked against the user's other positives, as in the
 *                        reference).  Counter-based: any window can be regenerated. */
int orx_sampler_stratified(orx_sampler* s, uint64_t seed, int64_t first, int64_t n, float pos_ratio,
                           int32_t* uid_dev, int32_t* iid_dev, float* label_dev);
int orx_sampler_per_pos_stratified(orx_sampler* s, uint64_t seed, int64_t first, int64_t n, double pos_ratio,
                                   int32_t* uid_dev, int32_t* iid_dev, float* label_dev);

/* ---- DLRM (recommenders/dlrm.py:6-100, modules/multi_layer_perceptron.py:5-18,
 * modules/second_order_feature_interaction.py:4-34; train step as in
 * tf2_examples/dlrm_criteo.py:42-48).  The n_emb embedding tables (all of dim
 * m_spa) live in ONE combined table, table f starting at row sum(ln_emb[0:f]).
 * The bottom MLP must end at m_spa (its output is stacked with the embeddings). */
typedef struct orx_dlrm orx_dlrm;
enum orx_dlrm_flags {
    ORX_DLRM_INTERACT_ITSELF = 1,   /* arch_interaction_itself                           */
    ORX_DLRM_SIGMOID_BOT = 2,       /* sigmoid_bot (else relu), dlrm.py:34-35            */
    ORX_DLRM_SIGMOID_TOP = 4,       /* sigmoid_top (else relu), dlrm.py:36-37            */
    ORX_DLRM_LOSS_BCE = 8,          /* loss_func='bce' (else 'mse'), dlrm.py:52-55       */
    ORX_DLRM_FP16_MLP = 32,         /* performance mode: the MLP products run on fp16 MFMA
                                       (operands rounded to fp16, fp32 accumulate / storage);
                                       NOT within the 1e-5 parity tolerance                 */
    ORX_DLRM_REFERENCE_COMPAT = 16, /* reproduce second_order_feature_interaction.py:21-32
                                       literally: lower triangle kept, upper selected -> the
                                       interaction output is 0; without this
                                       flag the strictly lower triangle is used             */
    ORX_DLRM_NO_EMB = 64            /* the model owns no embedding table: the rows come from
                                       outside (row-sharded tables, orx_dlrm_grads)         */
};
enum orx_dlrm_param_kind { ORX_DLRM_EMB = 0, ORX_DLRM_BOT_W = 1, ORX_DLRM_BOT_B = 2, ORX_DLRM_TOP_W = 3, ORX_DLRM_TOP_B = 4 };

int orx_dlrm_create(orx_ctx* ctx, int32_t m_spa, int32_t n_emb, const int64_t* ln_emb,
                    int32_t n_bot, const int32_t* ln_bot, int32_t n_top, const int32_t* ln_top,
                    int32_t dense_dim, int flags, float loss_threshold, uint64_t seed, orx_dlrm** out);
int orx_dlrm_destroy(orx_dlrm* m);
/* borrowed handle of a parameter: the combined embedding table, or Dense layer `layer`'s
 * kernel [in, out] / bias [1, out] (Keras layout).  Owned by the model. */
int orx_dlrm_param(orx_dlrm* m, int kind, int layer, orx_table** out);
/* K train steps (DLRM.call + tape.gradient + apply_gradients).  dense [K*B, dense_dim] fp32,
 * sparse [K*B, n_emb] int32 (id within its own table), label [K*B] fp32; host pointers unless
 * ORX_IDS_DEVICE.  loss_out: host float[K] or NULL. */
int orx_dlrm_step(orx_dlrm* m, orx_opt* opt, const float* dense, const int32_t* sparse, const float* label,
                  int64_t K, int64_t B, int flags, float* loss_out);
/* DLRM.inference (dlrm.py:76-100): pred_out host/device float[B] */
int orx_dlrm_inference(orx_dlrm* m, const float* dense, const int32_t* sparse, int64_t B, int flags, float* pred_out);
/* Hybrid-parallel train step (embedding tables row-sharded across ranks, MLPs data-parallel;
 * no reference equivalent).  All pointers are DEVICE pointers.
 *   orx_dlrm_grads       : forward + backward of this rank's B samples with the embedding rows
 *                          handed in (emb_rows [B, n_emb, m_spa], already exchanged); the loss
 *                          mean runs over global_B samples.  Writes d loss / d emb_rows to
 *                          emb_grads [B, n_emb, m_spa], leaves the dense gradients inside the
 *                          model and adds this rank's part of the loss to loss_accum[0] (double).
 *   orx_dlrm_dense_count : number of fp32 dense parameters (all kernels and biases)
 *   orx_dlrm_dense_pack  : copy the dense gradients into flat[count] (for ONE all-reduce)
 *   orx_dlrm_dense_apply : optimizer step of every dense parameter with the gradients in
 *                          flat[count] (after the all-reduce); advances the step counter. */
int orx_dlrm_grads(orx_dlrm* m, const float* dense, const float* emb_rows, const float* label, int64_t B,
                   int64_t global_B, float* emb_grads, double* loss_accum);
/*   orx_dlrm_grads_indirect : the same with the embedding rows read IN PLACE from the buffer the exchange filled (rows
 *                          [n_rows][m_spa], idx[b (n_emb + 1) + f] = row of lookup f of sample b, slot n_emb unused) and the
 *                          gradient of each lookup written to row idx[...] of grads_dst, the buffer that travels back: no
 *                          reordering passes.  orx_dlrm_direct_ok: 1 if this model's shapes allow it. */
int orx_dlrm_direct_ok(orx_dlrm* m);
/* The DLRM modules called on PLAIN ARRAYS (outside the composition dlrm.py:76-100, which is orx_dlrm_step / orx_dlrm_inference):
 *   orx_mlp_forward      openrec/tf2/modules/multi_layer_perceptron.py:5-18: y = act_L(... act_1(x W_1 + b_1) ...); kernels[l] is a
 *                        table [in_l, out_l] (Keras Dense layout), biases[l] a table [1, out_l] or NULL (biases may be NULL altogether),
 *                        acts[l] 0 none / 1 relu / 2 sigmoid; x [B, in_dim] -> y_out [B, out_L]; exact fp32 products.
 *   orx_interact_forward openrec/tf2/modules/second_order_feature_interaction.py:12-34: z [B, F, d] = the F inputs stacked on axis 1,
 *                        out [B, P], P = F (F - 1) / 2 (self_interaction: F (F + 1) / 2), the selected elements of Z Z^T in
 *                        boolean_mask order; reference_compat != 0 reproduces the reference's text (zeros: SURVEY.md E.1).
 * flags & ORX_IDS_DEVICE: x / z and the output are device pointers (asynchronous on the context's stream); otherwise host pointers. */
int orx_mlp_forward(orx_ctx* ctx, int32_t n_layers, orx_table* const* kernels, orx_table* const* biases, const int32_t* acts,
                    const float* x, int64_t B, int32_t in_dim, int flags, float* y_out);
int orx_interact_forward(orx_ctx* ctx, const float* z, int64_t B, int32_t F, int32_t d, int self_interaction, int reference_compat,
                         int flags, float* out);
int orx_dlrm_grads_indirect(orx_dlrm* m, const float* dense, const float* rows, int64_t n_rows, const int32_t* idx,
                            const float* label, int64_t B, int64_t global_B, float* grads_dst, double* loss_accum);
int orx_dlrm_dense_count(orx_dlrm* m, int64_t* count);
int orx_dlrm_dense_pack(orx_dlrm* m, float* flat);
int orx_dlrm_dense_apply(orx_dlrm* m, orx_opt* opt, const float* flat);

/* ---- sharded building blocks (row-wise sharded tables, one rank per GPU;
 * the exchange itself is RCCL all-to-all driven by the host, see
 * openrec_amd/sharded.py).  No reference equivalent (the reference is single
 * process).  All pointers are DEVICE pointers; ids are LOCAL row ids, an id < 0
 * marks a padding slot and is skipped.
 *   gather_rows : out[k, 0:D] = W[ids[k]], out[k, D] = bias[ids[k]] (bias may be NULL)
 *   pair_grads  : from gathered rows [T, row_stride] (bias at column D) compute the
 *                 per-occurrence gradients of J (bias gradient at column D of gp/gn)
 *                 and ADD this rank's (loss, l2_loss) contribution to loss_l2_accum[2];
 *                 the loss mean is taken over B_global; triplet k is live iff
 *                 valid == NULL or valid[k] >= 0
 *   apply_rows  : optimizer sparse apply of per-occurrence gradient rows
 *                 (SGD: every occurrence accumulated; Adagrad / Adam: duplicates summed first;
 *                 Adam takes the step the optimizer's counter stands at: orx_dlrm_dense_apply
 *                 advances it once per step, otherwise the host does with orx_opt_advance)
 */
int orx_gather_rows(orx_ctx* ctx, orx_table* t, orx_table* bias, const int32_t* ids, int64_t n,
                    float* out, int64_t out_stride);
int orx_pair_grads(orx_ctx* ctx, int model, int32_t D,
                   const float* u_rows, const float* p_rows, const float* n_rows, int64_t row_stride,
                   const int32_t* valid, int64_t T, int64_t B_global, float margin, int flags,
                   float* gu, float* gp, float* gn, int64_t g_stride, double* loss_l2_accum);
int orx_apply_rows(orx_ctx* ctx, orx_opt* opt, orx_table* t, orx_table* bias,
                   const int32_t* ids, int64_t n, const float* grads, int64_t g_stride);
/* K-step plans know every id list up front: duplicate flags of K lists in one launch
 * (dflag[k*n + i] = 1 iff row ids[k*id_stride + i] occurs more than once in list k), and the SGD
 * apply that uses them: rows referenced once are plain read-modify-writes, only duplicated rows
 * take atomics.  Same result as orx_apply_rows. */
int orx_rows_dupflags(orx_ctx* ctx, int64_t rows, const int32_t* ids, int64_t K, int64_t n, int64_t id_stride,
                      unsigned char* dflag);
int orx_apply_rows_flagged(orx_ctx* ctx, orx_opt* opt, orx_table* t, orx_table* bias, const int32_t* ids, int64_t n,
                           const float* grads, int64_t g_stride, const unsigned char* dflag);

/* Device-side exchange plan of the sharded step (openrec_amd/sharded.py): fixed-capacity
 * buckets, no host synchronization.  Row r of a table lives on rank r % world at local
 * index r / world.  `overflow` is a device int set to 1 when a bucket was full.
 *   shard_route   : triplets -> send[world*cap][3] (bucket = uid % world); fills unused slots with -1
 *   shard_request : received triplets [T][3] (u < 0 = empty) -> item-id requests
 *                   send_ids[world*cap] (bucket = id % world, -1 unused), slot[2T] (where the p / n
 *                   request of triplet t went, -1 if none) and u_loc[T] (local user row or -1)
 *   shard_localize: out[i] = ids[i] / world (or -1)
 *   shard_grads   : user rows from the local shard + received item rows [world*cap][DS] ->
 *                   gu[T][D] and the item-row gradients written in place into send_g at the slots
 *                   of their requests; adds the (loss, l2_loss) contribution to loss_l2_accum[2] */
int orx_shard_route(orx_ctx* ctx, const int32_t* uid, const int32_t* pid, const int32_t* nid, int64_t B,
                    int64_t users_global, int64_t items_global, int32_t world, int32_t cap,
                    int32_t* send, int32_t* counters, int32_t* overflow);
int orx_shard_request(orx_ctx* ctx, const int32_t* trip, int64_t T, int32_t world, int32_t cap,
                      int32_t* send_ids, int32_t* slot, int32_t* u_loc, int32_t* counters, int32_t* overflow);
/* the same two plans for K steps in one launch each (the plan depends on the ids alone): uid/pid/nid
 * [K][id_stride], send [K][world*cap][3], trip [K][T][3], send_ids [K][world*cap], slot [K][2T],
 * u_loc [K][T], counters [K][world] */
int orx_shard_route_steps(orx_ctx* ctx, const int32_t* uid, const int32_t* pid, const int32_t* nid, int64_t K, int64_t B,
                          int64_t id_stride, int64_t users_global, int64_t items_global, int32_t world, int32_t cap,
                          int32_t* send, int32_t* counters, int32_t* overflow);
int orx_shard_request_steps(orx_ctx* ctx, const int32_t* trip, int64_t K, int64_t T, int32_t world, int32_t cap,
                            int32_t* send_ids, int32_t* slot, int32_t* u_loc, int32_t* counters, int32_t* overflow);
int orx_shard_localize(orx_ctx* ctx, const int32_t* ids, int64_t n, int32_t world, int32_t* out);
/* generic request plan (hybrid-parallel DLRM lookups): every id >= 0 claims a slot in the bucket of its
 * owner rank (id % world): send_ids[world*cap] (-1 = empty), slot[n] = position in send_ids or -1;
 * counters[world] scratch, overflow[1] sticky flag (a bucket was full: that id is dropped) */
int orx_shard_bucket(orx_ctx* ctx, const int32_t* ids, int64_t n, int32_t world, int32_t cap,
                     int32_t* send_ids, int32_t* slot, int32_t* counters, int32_t* overflow);
/* orx_shard_request_steps with PER-DESTINATION DEDUP: an item that several references of a list ask for claims one slot of its
 * owner's bucket (its row travels once, the sum of the references' gradients travels back).  The distinct items of an owner fill
 * its bucket in ascending row order (a stable sort of the references by (owner, row): deterministic).  Outputs besides
 * send_ids / slot / u_loc: dupref[K][2T] = 1 on the references that share their slot; sorted_out [K][2T] x 8 bytes (the sorted
 * (key, reference) list), seglist [K][T] x 8 bytes and segcount [K] (the shared slots): opaque, handed back to orx_shard_grads.
 * items_global: rows of the global item table. */
int orx_shard_request_dedup_steps(orx_ctx* ctx, const int32_t* trip, int64_t K, int64_t T, int32_t world, int32_t cap,
                                  int64_t items_global, int32_t* send_ids, int32_t* slot, int32_t* u_loc, uint8_t* dupref,
                                  void* sorted_out, void* seglist, int32_t* segcount, int32_t* overflow);
/* dupref == NULL: every reference has a slot of its own.  Otherwise the list's outputs of orx_shard_request_dedup_steps and a side
 * buffer gdup [2T][row_stride]: references that share a slot leave their gradients there and a second launch writes the slot's
 * SUM, taken in reference order (no atomics: the result does not depend on timing). */
int orx_shard_grads(orx_ctx* ctx, int model, orx_table* user, const float* rows_in, const int32_t* u_loc,
                    const int32_t* slot, const uint8_t* dupref, const void* sorted, const void* seglist, const int32_t* segcount,
                    float* gdup, int64_t T, int64_t row_stride, int64_t B_global, float margin, int flags,
                    float* gu, float* send_g, double* loss_l2_accum);
/* orx_shard_grads with SGD's apply of the local user rows folded in (row-sharded BPR / UCML step, phases 4 + 5 of
 * openrec_amd/sharded.py; the reference's single-process apply is tf2_examples/bpr_citeulike.py:38): a user row referenced
 * once in the step is updated in place; the references of a duplicated row leave gu[t] and u_apply[t] = local row for
 * orx_apply_rows_flagged (u_apply[t] = -1 elsewhere).  dup_u[T]: orx_rows_dupflags of u_loc. */
int orx_shard_grads_sgd(orx_ctx* ctx, int model, orx_opt* opt, orx_table* user, const float* rows_in, const int32_t* u_loc,
                        const int32_t* slot, const uint8_t* dupref, const void* sorted, const void* seglist, const int32_t* segcount,
                        float* gdup, const uint8_t* dup_u, int64_t T, int64_t row_stride, int64_t B_global,
                        float margin, int flags, float* gu, int32_t* u_apply, float* send_g, double* loss_l2_accum);

/* ---- the row-sharded pairwise step as one host call (the single-process step it shards is
 * tf2_examples/bpr_citeulike.py:27-39).  Row r of every table lives on rank r % world at local index r / world; the ranks'
 * batches together are ONE global batch (loss mean over world * B).  An orx_comm wraps an RCCL communicator (librccl.so is
 * loaded at run time by orx_comm_create; the exchanges are ncclSend / ncclRecv groups on the context's stream) and owns the
 * exchange buffers of the engine.
 *   orx_comm_unique_id : rank 0 makes the 128-byte id (ncclGetUniqueId) and hands it to the other ranks by any means
 *   orx_comm_create    : collective over the ranks (ncclCommInitRank).  unique_id == NULL with world 1: a one-rank
 *                        communicator without RCCL (every exchange is the identity)
 *   orx_sharded_pairwise_steps : K steps of this rank's uid / pid / nid [K][id_stride] (DEVICE int32, B ids per step) on its
 *                        shards U / V / b.  The exchange plan (triplets -> owner of the user row, item ids -> owners) is made
 *                        for plan_chunk steps at a time with one exchange per phase; a step is then gather -> exchange (rows)
 *                        -> gradients -> apply users -> exchange (gradients) -> apply items.  Buckets have a fixed capacity
 *                        (mean * slack + 6 sigma + 16, orx_sharded_caps): `overflow` (device int, sticky) reports a full one.
 *                        loss_l2_accum: device double[2], this rank's (sum of loss, sum of l2_loss) contributions are added.
 *                        flags: ORX_NO_L2; ORX_SHARD_OVERLAP (needs id_stride == B, B even, a communicator with RCCL): every
 *                        step is cut into two half-batches whose exchanges run on a second stream beside the other half's
 *                        kernels.  Same results as the per-phase entry points driven by openrec_amd/sharded.py. */
#define ORX_COMM_ID_BYTES 128
#define ORX_SHARD_OVERLAP 0x100
#define ORX_SHARD_NO_DEDUP 0x200   /* every item reference claims a slot of its own (orx_shard_request_steps) */
#define ORX_SHARD_DEDUP 0x400      /* per-destination dedup of the item requests (orx_shard_request_dedup_steps); neither flag: on
                                    * when a list's item references number at least half the items (most slots are then shared) */
typedef struct orx_comm orx_comm;
int orx_comm_unique_id(void* id_out);
int orx_comm_create(orx_ctx* ctx, const void* unique_id, int32_t rank, int32_t world, orx_comm** out);
int orx_comm_destroy(orx_comm* comm);
/* An in-process group of `world` ranks that share ONE device -- one host thread and one context per rank, exchanges meeting at
 * a host barrier, blocks copied by kernels: the engine's complete exchange schedule with world > 1 where there is no second GPU
 * (tests/test_gpu_shard_engine.py).  orx_vgroup_abort releases ranks waiting for one that failed. */
typedef struct orx_vgroup orx_vgroup;
int orx_vgroup_create(int32_t world, orx_vgroup** out);
int orx_vgroup_abort(orx_vgroup* group);
int orx_vgroup_destroy(orx_vgroup* group);
int orx_comm_create_virtual(orx_ctx* ctx, orx_vgroup* group, int32_t rank, orx_comm** out);
int orx_comm_rank(orx_comm* comm);
int orx_comm_world(orx_comm* comm);
/* Measurement of the exchanges (bench.py --gpus N: phases_us / link_GBps).
 *   orx_comm_stats(comm, 1, NULL): start counting, counters at zero (HIP events around every exchange from now on);
 *   orx_comm_stats(comm, 0, out) : stop; out[0] = exchanges, out[1] = bytes this rank SENT to other ranks, out[2] = their device
 *                                  time in ms (sum over the exchanges, each timed on the stream it ran on), out[3] = bytes of the
 *                                  rank's own blocks (device copies, not on the wire).
 *   orx_comm_ping(comm, bytes, reps, out): `reps` all-to-alls of `bytes` per peer (ncclSend / ncclRecv to every other rank at once,
 *                                  as the engine's exchanges do) on fresh buffers; out[0] = GB/s this rank sent (all links together),
 *                                  out[1] = GB/s per link, out[2] = microseconds per all-to-all.  Collective: every rank calls it.
 *                                  A one-rank RCCL communicator measures the device copy of its own block; one made WITHOUT RCCL
 *                                  (every exchange is the identity) has nothing to time: out = {0, 0, 0}. */
int orx_comm_stats(orx_comm* comm, int start, double* out4);
int orx_comm_ping(orx_comm* comm, int64_t bytes, int32_t reps, double* out3);
int orx_sharded_caps(int64_t B, int32_t world, float slack, int64_t* cap1, int64_t* cap2);
/* the regrouping the engine applies around the plan's exchanges: src [K][world][words] -> dst [world][K][words] 4-byte words
 * (back != 0: the inverse); device pointers */
int orx_shard_regroup(orx_ctx* ctx, const void* src, void* dst, int64_t K, int32_t world, int64_t words, int back);
int orx_sharded_pairwise_steps(orx_comm* comm, orx_opt* opt, int model, orx_table* user, orx_table* item, orx_table* bias,
                               const int32_t* uid, const int32_t* pid, const int32_t* nid, int64_t K, int64_t B, int64_t id_stride,
                               int64_t users_global, int64_t items_global, float margin, float slack, int32_t plan_chunk,
                               int flags, double* loss_l2_accum, int32_t* overflow);
/* The same with HOT-ITEM REPLICATION (skewed item popularity): items 0 .. hot_items-1 of a vocabulary sorted by
 * popularity live in the replica tables item_hot [hot_items, D] / bias_hot [hot_items, 1], identical on every rank (the caller fills
 * them from the owners' shards before the first call and writes them back when it wants the shards current: openrec_amd/sharded.py
 * load_hot / sync_hot).  References to those items read the local replica and put nothing on the wire; their gradients are summed
 * per item on the rank, then over the ranks by ONE all-reduce of the [hot_items, D + 4] block per step, and every rank applies the
 * same sums to its replica (the replicas stay identical).  Exact: TF sums the gradients of duplicate ids before the sparse apply.
 * cold_fraction in (0, 1]: the share of a list's item references expected NOT to be hot -- the exchanged buckets (which travel
 * whole: fixed capacities, no size exchange) are sized for that share, which is what takes the hot rows off the wire; a list with
 * more cold references than its buckets hold sets *overflow like any other overflow.  1.0: buckets as without replication.
 * hot_items = 0: orx_sharded_pairwise_steps.  At most 63 ranks.  ORX_SHARD_DEDUP is refused together with hot_items > 0
 * (ORX_ERR_ARG): the plan with the replica as a destination is the one without per-destination dedup.  As with every overflow,
 * a call that sets *overflow dropped references: the tables AND the replicas (whose summed block the dropped triplets' slots
 * still entered) are not the result of the steps any more -- restore from a checkpoint, raise `slack` / `cold_fraction`. */
int orx_sharded_pairwise_steps_hot(orx_comm* comm, orx_opt* opt, int model, orx_table* user, orx_table* item, orx_table* bias,
                                   orx_table* item_hot, orx_table* bias_hot, int64_t hot_items, float cold_fraction,
                                   const int32_t* uid, const int32_t* pid, const int32_t* nid, int64_t K, int64_t B, int64_t id_stride,
                                   int64_t users_global, int64_t items_global, float margin, float slack, int32_t plan_chunk, int flags,
                                   double* loss_l2_accum, int32_t* overflow);

/* The hybrid-parallel DLRM step as one host call (BASELINE.json configs[4]; the single-process step: recommenders/dlrm.py:63-100 under
 * tf2_examples/dlrm_criteo.py:42-48).  `emb` is this rank's shard of the COMBINED embedding table (row r of the concatenated tables
 * on rank r % world at local index r / world), `m` a model made with ORX_DLRM_NO_EMB (its MLPs are replicas), dense / sparse / label
 * this rank's K x B slice of the global batches (DEVICE pointers; sparse ids are ids within their own table).  Per step: lookups ->
 * owners (ncclSend / ncclRecv groups), rows back, forward + backward on the rows where they arrived, row gradients to the owners,
 * ONE ncclAllReduce of the packed dense gradients, applies.  loss_accum: device double[1], this rank's share of the global-batch
 * loss is added per step; overflow: device int, sticky (a request bucket -- mean * slack + 8 -- was full).  Same results as the
 * per-phase entry points (orx_shard_bucket, orx_gather_rows, orx_dlrm_grads_indirect, orx_dlrm_dense_pack / _apply, orx_apply_rows)
 * driven by openrec_amd/sharded_dlrm.py. */
int orx_sharded_dlrm_steps(orx_comm* comm, orx_dlrm* m, orx_opt* opt, orx_table* emb, const float* dense, const int32_t* sparse,
                           const float* label, int64_t K, int64_t B, float slack, double* loss_accum, int32_t* overflow);

/* ---- device-time sampling of the kernels (HIP events on the ctx stream) --- */
int orx_prof_enable(orx_ctx* ctx, int on);
int orx_prof_reset(orx_ctx* ctx);
/* total device milliseconds and launch count recorded for kernel `kid` */
int orx_prof_get(orx_ctx* ctx, int kid, double* total_ms, int64_t* launches);
/* What the plan of the most recent exact pairwise call counted (tests, diagnosis; waits for that call's counters if nobody has
 * looked at them yet -- see DESIGN.md 4.0 "no read-back"):
 *   what = 0  rows referenced exactly twice that were PAIRED (accepted pairs, summed over the call's steps)
 *        = 1  largest number of duplicated rows one step left for the apply
 *        = 2  pairwise calls so far that enqueued every launch without waiting for their plan's counters
 *        = 3  1 if those counters were "quiet" (no range wanted a staging plan, few duplicated rows), else 0 */
int orx_ctx_stat(orx_ctx* ctx, int what, int64_t* out);
/* The streaming-copy yardstick of this device (bench.py's `roofline.frac_of_copy_peak`; no reference equivalent): a float4 copy
 * kernel over two buffers of `bytes` each (allocated and released inside the call; bytes % 16 == 0), three untimed launches, then
 * `reps` timed ones on the context's stream; *gbps_out = 2 * bytes / mean launch time, in 1e9 bytes per second. */
int orx_copy_bandwidth(orx_ctx* ctx, int64_t bytes, int32_t reps, double* gbps_out);

/* ---- the fp16 MLP products alone (diagnostics and tests; no reference equivalent: the reference's Dense layers are TensorFlow's) ----
 * The launchers of the ORX_DLRM_FP16_MLP step on caller-owned DEVICE buffers, on the context's stream (order producers with
 * orx_ctx_wait_stream, read results after orx_synchronize).  fp16 operands are [rows][ld] halves with ld % 8 == 0 and 16-byte aligned
 * bases; the halves between the used columns and ld must be ZERO (the kernels multiply whole 16-byte chunks).  act / act_y: 0 none,
 * 1 relu, 2 sigmoid.  Shapes a kernel does not carry are refused with ORX_ERR_ARG, never run.
 *   orx_gemm16_plan     what the launchers choose on `num_cu` CUs (no device needed; the environment switches ORX_GEMM16_* of the process apply):
 *                       nt_out[8] for C[M][N] = A[M][K] B[N][K]^T: {tile config 1 = 256x128 / 2 = 128x128 / 3 = 128x64, stages 0 = register-staged /
 *                       2 / 3 = LDS-DMA, TAIL, wave tile, BM, BN, workgroups, mask words};  tn_out[8] for C[M][N] += A[K][M]^T B[K][N]:
 *                       {S slices, tiles, kchunk, form 0 = register-staged / 2 / 3 = LDS-DMA / 4 = two K groups, TAIL, 0, 0, 0}
 *   orx_gemm16_group_query  the grouped backward launch of a layer [B, out] -> [B, in]: plan_out[8] = {the DLRM step would group it, tn TAIL,
 *                       nt TAIL, S, tiles, kchunk, tn workgroups, nt workgroups}
 *   orx_gemm16_nt       C (fp32, optional) / C16 (fp16, optional) = epilogue(A16 B16^T): + bias[N], act; then, with actY (fp32) or actY16 (fp16)
 *                       [M][ldy], the fused activation backward v * act_y'(Y) and, with colparts, its column sums per row block:
 *                       colparts[P][N], *P_out = P = ceil(M / BM).  mask_out: one bit per output element "fp16 value > 0", mask words of
 *                       orx_gemm16_plan; mask_in: such a mask of the same [M][N] in place of reading actY16 (relu; LDS-DMA forms only)
 *   orx_gemm16_tn       C[M][N] += out_scale * A16[K][lda]^T B16[K][ldb]; slab: tiles * S * (128 * 128 + 64) floats when S > 1 (the entry then
 *                       runs the slab reduce as well and waits for it)
 *   orx_gemm16_group    both backward products of a layer in one launch: gW[in][out] += out_scale * X16[B][ldx]^T dZ16[B][lddz] and
 *                       C / C16 [B][nt_cols or in] = dZ16 W16[nt_cols or in][ldw]^T with the epilogue of orx_gemm16_nt (no bias, no act)
 *   orx_head16_fwd      pred[b] = act(bias[0] + X16[b][:K] . w16[:K])
 *   orx_head16_bwd      dz = dy * act'(pred); partial rows per workgroup (*P_out of them, at most orx_head16_bwd_blocks(ctx, B)):
 *                       gb_parts[P] (sum dz), gW_parts[P][K] (sum X dz16), gb_below_parts[P][K]; dZ16 (and dZ32, optional) [B][K] =
 *                       dz16 w16 act_below'(X16)
 *   orx_cast16          dst16[M][ld16] = fp16(src[M][lds] columns < N), round to nearest even; the columns N .. ld16 - 1 are set to zero */
int orx_gemm16_plan(int32_t num_cu, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb, int32_t* nt_out, int32_t* tn_out);
int orx_gemm16_group_query(int32_t num_cu, int32_t B, int32_t in, int32_t out, int64_t ldx, int64_t lddz, int64_t ldw, int32_t nt_cols,
                           int32_t* plan_out);
int orx_gemm16_nt(orx_ctx* ctx, const void* A16, int64_t lda, const void* B16, int64_t ldb, float* C, int64_t ldc, void* C16, int64_t ldc16,
                  const float* bias, int32_t M, int32_t N, int32_t K, int act, const float* actY, const void* actY16, int64_t ldy, int act_y,
                  float* colparts, int32_t* P_out, void* mask_out, const void* mask_in);
int orx_gemm16_tn(orx_ctx* ctx, const void* A16, int64_t lda, const void* B16, int64_t ldb, float* C, int64_t ldc, float* slab,
                  int32_t M, int32_t N, int32_t K, float out_scale);
int orx_gemm16_group(orx_ctx* ctx, const void* X16, int64_t ldx, const void* dZ16, int64_t lddz, float* gW, int64_t ldgw, float* slab,
                     int32_t in, int32_t out, int32_t B, float out_scale, const void* W16, int64_t ldw, float* C, int64_t ldc,
                     void* C16, int64_t ldc16, const float* actY, const void* actY16, int64_t ldy, int act_y, float* colparts,
                     int32_t* P_out, const void* mask_in, int32_t nt_cols);
int orx_head16_fwd(orx_ctx* ctx, const void* X16, int64_t ldx, const void* w16, const float* bias, int act, float* pred, int32_t B, int32_t K);
int32_t orx_head16_bwd_blocks(orx_ctx* ctx, int32_t B);
int orx_head16_bwd(orx_ctx* ctx, const void* X16, int64_t ldx, const void* w16, const float* dy, const float* pred, int act, int act_below,
                   float* gW_parts, float* gb_parts, void* dZ16, int64_t ld16, float* dZ32, int64_t ld32, float* gb_below_parts,
                   int32_t B, int32_t K, int32_t* P_out);
int orx_cast16(orx_ctx* ctx, const float* src, int64_t lds, void* dst16, int64_t ld16, int32_t M, int32_t N);

/* ---- alternating least squares for WRMF (beyond the reference API, whose wrmf.py trains by SGD over sampled points: the closed
 * form of Hu / Koren / Volinsky over ALL row x column cells).  One half-step holds `fixed` (F, rows f_j, [M, D]) and overwrites rows
 * [row0, row0 + nrows) of `solved` (X, [R, D]).  Row r has the observed columns O_r = cols[row_ptr[r] .. row_ptr[r + 1]) of a CSR
 * over ALL R rows of `solved` (row_ptr int64 [R + 1], cols int32, ascending and distinct inside a row); observation (r, j) has
 * preference 1 and confidence c_rj = conf[e] (a float array aligned with cols) or `a` for all of them when conf == NULL; every other
 * cell has preference 0 and confidence b.  There is no bias term.
 *     G   = F^T F                                              once per call
 *     A_r = b G + sum_{j in O_r} (c_rj - b) f_j f_j^T + reg I
 *     y_r = sum_{j in O_r} c_rj f_j
 *     x_r = A_r^-1 y_r                                         Cholesky in fp32; A_r is SPD for reg > 0, b >= 0, c_rj >= b
 * A row without observations becomes exact +0.0 without a solve.  The user half-step passes the user -> items CSR with fixed = the
 * item table, the item half-step the item -> users CSR with fixed = the user table; the two descend
 *     sum over all cells c (p - u.v)^2 + reg (|U|_F^2 + |V|_F^2).
 * Rows of more than orx_als_segment_len() entries are cut into segments of that many entries; each segment's partial (A, y) is formed
 * from zero and the row adds them in segment order.  No float atomics anywhere: x_r is a function of (F, the row's entries, a, b,
 * reg) alone -- bit for bit the same whatever the row range of the call, the other rows in it, the scratch available, or where the
 * CSR lives.
 *   flags          ORX_IDS_DEVICE: row_ptr, cols and conf are device pointers and the call runs on the context's stream without a
 *                  host synchronisation; else they are host arrays, the rows' part of them is copied over, and the call returns after
 *                  orx_check_index_error.
 *   conf values    are not validated (c_rj < b can make A_r indefinite); a non-finite value in F, conf or the scalars' products gives a
 *                  non-finite x_r and never a hang: no loop's trip count depends on a floating-point value.
 *   lazy Adam      both tables are brought up to date before they are read, as orx_score_all_items does; the optimizer slots of the
 *                  solved table are left as they are (an optimizer that trained it keeps its moments).
 * ORX_ERR_ARG before any launch, the tables untouched: fixed dim != solved dim or dim > 128; reg <= 0 or not finite; b < 0 or not
 * finite; conf == NULL and a < b or a not finite; fixed == solved; a table on another context than `ctx`; a row range outside
 * `solved`; unknown flags; a host row_ptr that decreases.  A column id outside [0, M) is dropped from its row and reported by
 * orx_check_index_error (at once with a host CSR).  nrows == 0: ORX_OK, nothing is launched. */
int32_t orx_als_segment_len(void);
int orx_als_half_step(orx_ctx* ctx, orx_table* fixed, orx_table* solved,
                      const int64_t* row_ptr, const int32_t* cols, const float* conf /* or NULL */,
                      int64_t row0, int64_t nrows, float a, float b, float reg, int flags);

/* The same half-step solved INEXACTLY by cg_steps steps of conjugate gradient started from the row's current value (Takacs /
 * Pilaszy / Tikk 2011): A_r is never formed and nothing is factorised.  The contract of a row:
 *     A v  :=  b (G v) + reg v + sum_{j in O_r} (c_j - b) (f_j . v) f_j
 *     x = the row's CURRENT value in `solved` (warm start);  r = y_r - A x;  p = r;  rs = r . r
 *     repeat cg_steps times:
 *         if rs <= 1e-20: the row is done, x stays            (a select that freezes the row, not a trip count)
 *         Ap = A p;  alpha = rs / (p . Ap);  x += alpha p;  r -= alpha Ap
 *         rsn = r . r;  p = r + (rsn / rs) p;  rs = rsn
 *     store x (fp32)
 * The sums behind A v and y_r are fp32; x, r and the scalars of the recurrence (rs, p . Ap, alpha, beta) with their D-length dot
 * products are fp64, p is rounded to fp32 for the product.  A row without observations stores exact +0.0.  Every loop's trip count is
 * an integer function of D, cg_steps and the row's length; NaN compares false in the guard and flows through: non-finite inputs give
 * non-finite rows and never a hang.  No float atomics: x_r is a function of (F, the row's entries and current value, a, b, reg,
 * cg_steps) alone -- the same bits whatever the call's row range, the other rows in the call, the order of calls, the scratch
 * available, or where the CSR lives.  The code path of a row depends on its length and D only; orx_als_cg_row_breaks writes the
 * lengths at which it changes (ascending, at most `cap` of them) and returns how many there are (0: none, or dim outside [1, 128]):
 * rows up to the first keep their gathered f_j in LDS across the products, longer ones stream them per product, rows beyond the last
 * are cut into segments of that many entries whose partials are formed by separate workgroups and added in segment order (a call
 * has scratch for 65536 segments, fewer with the environment variable ORX_ALS_CG_SLOTS; a row beyond it is walked by one
 * wavefront, segment by segment, to the same bits).
 * Arguments, flags, index errors, lazy Adam and the solved table's version as for orx_als_half_step; in addition cg_steps outside
 * [1, 128] is ORX_ERR_ARG before any launch. */
int orx_als_half_step_cg(orx_ctx* ctx, orx_table* fixed, orx_table* solved,
                         const int64_t* row_ptr, const int32_t* cols, const float* conf /* or NULL */,
                         int64_t row0, int64_t nrows, float a, float b, float reg, int32_t cg_steps, int flags);
int32_t orx_als_cg_row_breaks(int32_t dim, int32_t* out, int32_t cap);

/* The objective both half-steps descend, for the user -> items CSR over ALL rows of `user`:
 *     sum over all cells c (p - u.v)^2 + reg (|U|_F^2 + |V|_F^2)
 *       = b <G_U, G_V>_F + sum_{(u,i) observed} [ c (1 - s)^2 - b s^2 ] + reg (tr G_U + tr G_V),     s = u . v
 * from the two grams (fp32 slabs, added in fp64) and one pass over the CSR (s and everything after it in fp64).  Every reduction
 * across rows, tiles or workgroups is fp64 in a fixed order, there are no atomics: two calls give the same bits.  The call
 * synchronises and writes one double to *host_out.  Argument and index-error rules as for orx_als_half_step (a column outside the
 * item table is left out of the sum and reported); a non-finite value in a table or a confidence gives a non-finite result. */
int orx_als_objective(orx_ctx* ctx, orx_table* user, orx_table* item,
                      const int64_t* row_ptr, const int32_t* cols, const float* conf /* or NULL */,
                      float a, float b, float reg, int flags, double* host_out);

/* ---- graph propagation over a CSR (api_csr.hip, kernels_graph.hip; DESIGN.md "LightGCN") ------------------------------------
 * One half-layer of LightGCN's propagation.  For rows [row0, row0 + nrows) of a CSR over the rows of `out`, whose columns index
 * the rows of X:
 *     y[r]    = row_scale[r] * sum_{e in row r, in CSR order} col_scale[cols[e]] * X[cols[e]]          (fp32)
 *     out[r]  = y[r]
 *     acc[r] += acc_alpha * y[r]                                                                       (acc != NULL)
 * row_scale / col_scale are DEVICE arrays over all rows of out / X (NULL: 1).  An empty row writes exact +0.0 to out and leaves
 * acc alone.  Rows of more than orx_graph_segment_len() entries are cut into segments of that many entries, each summed from
 * zero by a wavefront of its own; the row adds the partial sums in segment order.  No float atomics anywhere: y[r] is a function
 * of (X, the row's entries, the scales) alone -- the same bits for any row range, any split into calls, any other rows in the
 * call, a host or a device CSR -- and the order in which a row's terms are added is a function of the row's length and the dim
 * alone.  No trip count depends on a float: non-finite inputs give non-finite outputs.
 *   long_segments   only read with a device CSR, where the host cannot see the row lengths: the number of segments of the CSR's
 *           rows of more than orx_graph_segment_len() entries, sum over those rows of ceil(n / segment_len), counted once by the
 *           caller (an upper bound serves every row range).  It sizes the scratch of the partial sums and, when 0, skips the plan
 *           and the segment launch altogether.  A count that is too small is safe: a long row that finds no scratch slot walks its
 *           segments itself, the same sums in the same order, the same bits.  < 0: unknown; the scratch is then sized from the
 *           rows of X (a row's columns are distinct), up to 256 MiB that stay reserved on the context.
 *   flags   ORX_IDS_DEVICE: row_ptr and cols are device pointers and the call runs on the context's stream without a host
 *           synchronisation; else they are host arrays, the rows' part is copied over and the call returns after
 *           orx_check_index_error.
 * ORX_ERR_ARG before any launch: X == out or X == acc or out == acc; dims that differ or lie outside [1, 128]; acc with other
 * rows than out; a row range outside out; a table on another context; unknown flags.  A column outside X is dropped from its
 * row and reported (ORX_ERR_INDEX from this call with a host CSR, from orx_check_index_error with a device CSR).  nrows == 0
 * launches nothing.  Lazily-applied Adam is finished on all three tables before they are touched. */
int32_t orx_graph_segment_len(void);
int orx_graph_spmm(orx_ctx* ctx, orx_table* X, orx_table* out, orx_table* acc /* or NULL */, float acc_alpha,
                   const int64_t* row_ptr, const int32_t* cols,
                   const float* row_scale /* or NULL */, const float* col_scale /* or NULL */,
                   int64_t row0, int64_t nrows, int64_t long_segments, int flags);

/* The Keras DENSE rule of `opt` on every element of `table` with the device gradient grad [rows][dim] (read only): SGD, momentum /
 * Nesterov, Adagrad, Adam.  Adam's counter advances by one first (other tables lazily applied under `opt` are finished and leave
 * the lazy set, as in orx_pairwise_step) and the step is taken at the new count; the table's lazily-applied Adam is finished
 * before, so afterwards every row is current at that step and the table can go to orx_pairwise_step and back. */
int orx_table_apply_dense(orx_ctx* ctx, orx_opt* opt, orx_table* table, const float* grad);

/* ---- LightGCN (api_lightgcn.hip) -------------------------------------------------------------------------------------------
 *     E(0) = [user ; item],  E(k+1) = A~ E(k) (k < layers),  E_f = sum_k layer_weights[k] E(k),
 *     A~[u, i] = user_scale[u] * item_scale[i] on observed (u, i), symmetric
 * The workspace keeps the layer tables, the propagated tables (user_final, item_final of orx_lightgcn_tables: ordinary tables of
 * this context, owned by the workspace, valid until the next step or propagate) and the gradient tables.  It does NOT own the
 * two CSRs (user -> items, item -> users: device arrays) and the two scale vectors (device, both NULL: a plain neighbour sum),
 * which must outlive it.  layer_weights: host float[layers + 1] or NULL for 1 / (layers + 1).
 *   propagate   (user, item) -> (user_final, item_final): 2 layers orx_graph_spmm calls with the layer sum fused through acc
 *   step        one BPR step (no item bias) on the propagated rows of the triplets uid / pid / nid [B]:
 *               loss = mean_B -log sigmoid(s_p - s_n),  l2 = l2_reg / B * sum_b (|user[u]|^2 + |item[p]|^2 + |item[n]|^2) / 2
 *               over the LAYER-0 rows.  The per-occurrence gradients are summed into dense tables by a stable sort and sums in
 *               position order, propagated by the same operator (backward = forward), the l2 gradient is added per occurrence,
 *               and the dense rule of `opt` is applied to user and item (train_mask: ORX_TRAIN_USER | ORX_TRAIN_ITEM, 0 = both;
 *               Adam's counter advances once).  No float atomics touch a table: two steps from one state give the same bits.
 *               loss_out == l2_out == NULL and ORX_IDS_DEVICE: no host synchronisation.
 *   loss        the forward alone -> (loss, l2); no table of the model changes.
 * ORX_ERR_ARG before any device work: layers outside [1, ORX_LIGHTGCN_MAX_LAYERS]; dims that differ or lie outside [1, 128];
 * user == item; a table or optimizer on another context; one scale vector without the other; l2_reg negative or not finite;
 * mask bits outside the two; unknown flags.  An id outside its table: ORX_ERR_INDEX as orx_pairwise_step reports it; the id is
 * never used as an address. */
#define ORX_LIGHTGCN_MAX_LAYERS 8
typedef struct orx_lightgcn orx_lightgcn;
int orx_lightgcn_create(orx_ctx* ctx, orx_table* user, orx_table* item,
                        const int64_t* user_ptr, const int32_t* user_cols, const int64_t* item_ptr, const int32_t* item_cols,
                        const float* user_scale /* or NULL */, const float* item_scale /* or NULL */,
                        int64_t user_long_segments, int64_t item_long_segments /* as orx_graph_spmm's, per CSR; < 0: unknown */,
                        int32_t layers, const float* layer_weights /* or NULL */, orx_lightgcn** out);
int orx_lightgcn_destroy(orx_lightgcn* g);
int orx_lightgcn_tables(orx_lightgcn* g, orx_table** user_final, orx_table** item_final);
int orx_lightgcn_propagate(orx_lightgcn* g);
int orx_lightgcn_step(orx_lightgcn* g, orx_opt* opt, const int32_t* uid, const int32_t* pid, const int32_t* nid, int64_t B,
                      float l2_reg, int train_mask, int flags, float* loss_out, float* l2_out);
int orx_lightgcn_loss(orx_lightgcn* g, const int32_t* uid, const int32_t* pid, const int32_t* nid, int64_t B,
                      float l2_reg, int flags, float* loss_out, float* l2_out);

/* ---- VBPR (api_vbpr.hip, kernels_vbpr.hip): BPR with item content features through a learned projection (He & McAuley, AAAI 2016).
 * Tables: user [NU, D] with D = Dl + Dc (columns [0, Dl) = U_l, [Dl, D) = U_c); item [NI, Dl]; bias [NI, 1] or NULL; proj = E [Fd, Dc],
 * a table like the others; F [NI, Fd]: fixed fp32 item features, a DEVICE pointer, row-major, never written.
 *   theta_i = F[i] E
 *   s(u, i) = U_l[u] . V[i] + U_c[u] . theta_i + b[i]
 *   x_k     = s(u_k, p_k) - s(u_k, n_k) = U_l[u] . (V[p] - V[n]) + U_c[u] . ((F[p] - F[n]) E) + b[p] - b[n]
 *   loss    = (1/B) sum_k w_k * -log_sigmoid(max(x_k, -30))            w_k = weight[s*id_stride + k], 1 when weight == NULL
 *   l2_loss = 1/2 (sum_k |U[u_k]|^2 + |V[p_k]|^2 + |V[n_k]|^2)         the whole user row; no biases; never weighted
 *   J       = loss + l2_reg * l2_loss + l2_proj * 1/2 |E|_F^2
 * The projection has NO output bias (the reference's Dense layer has one): it cancels in every pair difference, its loss gradient is
 * identically zero, and in serving it shifts all items of a user equally.  No activation, one layer.
 * loss_out[s] is the loss, l2_out[s] the UNSCALED l2_loss of the rows (the caller forms J).  Gradients, per occurrence and on the
 * pre-step tables, with g_k = -w_k sigmoid(-x_k) [x_k >= -30] / B, df_k = F[p_k] - F[n_k], Delta_k = df_k E:
 *   g_U[k] = [ g_k (V[p] - V[n]) ; g_k Delta_k ] + l2_reg U[u]
 *   g_V[p] = g_k U_l[u] + l2_reg V[p],   g_V[n] = -g_k U_l[u] + l2_reg V[n],   g_b[p] = g_k,   g_b[n] = -g_k
 *   dE     = sum_k df_k^T (g_k U_c[u_k]) + l2_proj E                   [Fd, Dc], dense
 * Both products over feature rows are fp32 MFMA products: every product is rounded once into an fp32 fma chain, no float atomics;
 * dE is summed over chunks of the batch in chunk order, so the same state gives the same bits of dE.
 *   orx_features_project   out[k*out_stride + out_col0 + c] = ((F[ia[k]] - F[ib[k]]) E)[c], c < Dc, k < n.  ib == NULL: no subtraction;
 *                          ia == NULL: rows row0 + k.  out: a DEVICE pointer; other columns of its rows are not touched.  ia / ib are
 *                          host arrays unless ORX_IDS_DEVICE.  An id outside [0, NI) sets the index error and zeroes its output row.
 *   orx_vbpr_item_table    rows [row0, row0 + nrows) of W [NI, Dl + Dc]: columns [0, Dl) = item bit for bit, [Dl, D) = F E.  (user, W,
 *                          bias) then go to the scorers, top-K, the metrics and the candidate paths as BPR's tables do.
 *   orx_vbpr_step          K steps.  Per step: lazily-applied rows the step reads are brought up to date (user with uid, item and bias
 *                          with pid and nid), the projection, the pass over the triplets, the projection gradient; Adam's counter
 *                          advances once, after the reads and before the applies; orx_apply_rows of user with uid, of item and of bias
 *                          with pid | nid (each as a table of its own: the sorted apply, so a table's bits do not depend on the mask);
 *                          the dense rule on E at the step's count (E is synced first).  A K-step call is K one-step calls, bit for
 *                          bit.  loss_out == l2_out == NULL with ORX_IDS_DEVICE: no host synchronisation.
 *                          train_mask: ORX_TRAIN_USER | _ITEM | _BIAS | _PROJ, 0 = every table the call was given; a table outside
 *                          the mask is read, never written, and its optimizer slots are untouched.
 *                          batch_chunk: rows of the batch per partial of dE; 0 = the launcher's own choice from (B, Fd, Dc), else a
 *                          positive multiple of 64.  flags: ORX_IDS_DEVICE, ORX_NO_L2 (then l2_reg == l2_proj == 0).
 *   orx_vbpr_loss          the forward alone: (loss, l2_loss) of one batch, the step's numbers bit for bit; no table changes.
 *   orx_vbpr_geometry      host only: out = { rows of the batch per chunk, chunks, Dc padded to the tile width, rows of E per workgroup }.
 * ORX_ERR_ARG before any device work: Dl < 1; Dc outside [1, 128]; Dl + Dc > 256 or != the user dim; Fd outside [1, 8192] or != E's
 * rows; B >= 2^31 - 256; NI != the item rows; a bias that is not [NI, 1]; l2_reg / l2_proj negative or not finite; ORX_NO_L2 with a
 * coefficient != 0; ORX_HOGWILD, ORX_CENSOR; batch_chunk negative or no multiple of 64; mask bits outside the four; ORX_TRAIN_BIAS
 * with bias == NULL; tables or optimizer on another context; what orx_apply_rows refuses (ORX_ADAM_DENSE with a bias).
 * An id outside its table: ORX_ERR_INDEX as orx_multineg_step reports it; the id is never used as an address and its triplet
 * contributes no loss, no l2 and no gradient.  NaN features propagate to exactly the outputs that depend on their row. */
enum orx_vbpr_train_mask { ORX_TRAIN_PROJ = 8 };      /* a fourth bit beside orx_train_mask's three: the projection E */
int orx_features_project(orx_ctx* ctx, const float* F, int64_t NI, int32_t Fd, orx_table* proj,
                         const int32_t* ia /* NULL ok */, const int32_t* ib /* NULL ok */, int64_t row0, int64_t n,
                         float* out, int64_t out_stride, int32_t out_col0, int flags);
int orx_vbpr_item_table(orx_ctx* ctx, orx_table* item, orx_table* proj, const float* F, int64_t NI, int32_t Fd,
                        int64_t row0, int64_t nrows, orx_table* W);
int orx_vbpr_step(orx_ctx* ctx, orx_opt* opt, orx_table* user, orx_table* item, orx_table* bias /* NULL ok */, orx_table* proj,
                  const float* F, int64_t NI, int32_t Fd,
                  const int32_t* uid, const int32_t* pid, const int32_t* nid, const float* weight /* NULL ok */,
                  int64_t K, int64_t B, int64_t id_stride, float l2_reg, float l2_proj, int32_t batch_chunk, int train_mask, int flags,
                  float* loss_out, float* l2_out);
int orx_vbpr_loss(orx_ctx* ctx, orx_table* user, orx_table* item, orx_table* bias /* NULL ok */, orx_table* proj,
                  const float* F, int64_t NI, int32_t Fd,
                  const int32_t* uid, const int32_t* pid, const int32_t* nid, const float* weight /* NULL ok */,
                  int64_t B, int flags, float* loss_out, float* l2_out);
int orx_vbpr_geometry(int64_t B, int32_t Fd, int32_t Dc, int32_t batch_chunk, int32_t out[4]);

/* ---- History-pooled sequence recommender (api_seqrec.hip, kernels_bag.hip): the user vector is pooled from the embeddings of the
 * items the user just interacted with, so there is no user table and a user never trained on is served from a history alone
 * (the depth-0 YouTube retrieval tower, FISM, item2vec).
 * Tables: hist = H [NI, D], item = V [NI, D], bias [NI, 1] or NULL; D <= 256.  Bags in ragged form, the (input, offsets) form of an
 * EmbeddingBag: bag_ptr int32 [B + 1], bag_items int32 [n], bag i = bag_items[bag_ptr[i] .. bag_ptr[i + 1]); n is the length of
 * bag_items.  Both arrays live where the ids live (host, or device under ORX_IDS_DEVICE).  Contract: bag_ptr[0] == 0, non-decreasing,
 * bag_ptr[B] == n, n < 2^31.
 *   q_i     = c_i * sum over e in bag i, in list order, of H[bag_items[e]]
 *             c_i = 1.0f / (float)len_i (ORX_BAG_MEAN)  |  1.0f / denom (ORX_BAG_FIXED; denom = 1: a sum, denom = max_seq_len: a
 *             mean over a padded axis)
 *   s(q, j) = q . V[j] + b[j]
 * The sum is an fp32 chain whose order depends on (len_i, D) alone; c_i is rounded once, the product once; an empty bag gives +0.
 * The bits of q_i depend on its own list and on H: not on B, not on the other bags, not on out_row0, not on where the lists live.
 * No float atomics.
 *   orx_bag_pool      rows [out_row0, out_row0 + B) of out (another table of H's dim) = q_i; nothing else is touched.  Rows of H that
 *                     are lazily applied under Adam are brought up to date first.  ORX_IDS_DEVICE: no host synchronisation (a bad
 *                     list then shows at the next orx_check_index_error).
 *   orx_seqrec_step   ONE train step of orx_multineg_step's objective with u_i replaced by q_i: kinds ORX_MN_SOFTMAX / ORX_MN_LOGSIG,
 *                     N in [1, 64] negatives per sample, weight [B], neg_offset [B][N] as there.
 *                       l2_loss = 1/2 (sum_i |q_i|^2 + sum |V[p]|^2 + sum |V[n]|^2);   J = loss + l2_reg * l2_loss
 *                     The l2 term sits on the POOLED vector, not on the len_i history rows (the reference's l2_reg_embed sits on the
 *                     looked-up rows).  With g_q[i] = orx_multineg_step's g_u of sample i, occurrence e of bag i has the gradient row
 *                     c_i * g_q[i], each element rounded once, and hist is applied with orx_apply_rows' semantics on the list
 *                     bag_items[n] with those rows: a row's occurrences are summed in list order, the rule runs once per distinct row.
 *                     The n x D occurrence rows are never materialised: scratch is O(n) words plus O(B (1 + N) D).  item and bias
 *                     are applied exactly as orx_multineg_step applies them (one list, pid | nid).  Adam's counter advances once,
 *                     after the reads and before the applies.  loss_out / l2_out: the loss and the UNSCALED l2_loss; both NULL with
 *                     ORX_IDS_DEVICE: no host synchronisation.
 *                     train_mask: ORX_TRAIN_USER (the history table) | _ITEM | _BIAS, 0 = every table the call was given; a table
 *                     outside the mask is read, never written, and its optimizer slots are untouched.  flags: ORX_IDS_DEVICE, ORX_NO_L2.
 *   orx_seqrec_loss   the forward alone: (loss, l2_loss) of one batch, the step's numbers bit for bit; no table changes.
 * ORX_ERR_ARG before any device work: hist and item the same table, or their dims or rows differ; dim > 256; a bias that is not
 * [NI, 1]; a mode outside the two; denom not finite or <= 0; N outside [1, 64]; l2_reg negative or not finite; ORX_NO_L2 with
 * l2_reg != 0; ORX_HOGWILD, ORX_CENSOR; what orx_apply_rows refuses (ORX_ADAM_DENSE with a bias); B outside [0, 2^31 - 1), n outside
 * [0, 2^31), B (1 + N) >= 2^31; a host bag_ptr that breaks the contract; out rows outside the output table, out == H.
 * A device bag_ptr that breaks the contract, or an item id outside [0, NI) in a bag, in pid or in nid: ORX_ERR_INDEX (host lists:
 * from the call; device lists: from the call when it returns losses, else at the next orx_check_index_error).  The id is never used
 * as an address, a bag that holds one pools to +0 and its sample is dropped, and the context stays usable; the tables are then
 * only guaranteed to be in bounds and finite.
 * Not offered: tied tables (hist == item); per-occurrence weights (recency decay); the reference's hidden Dense(D) layer and
 * dropout; in-batch negatives; K-step calls (a step at realistic sizes is hundreds of microseconds); the sharded engines.
 * (The full softmax over all items is orx_seqrec_full_step, below.) */
enum orx_bag_mode { ORX_BAG_MEAN = 0, ORX_BAG_FIXED = 1 };
int orx_bag_pool(orx_ctx* ctx, orx_table* H, const int32_t* bag_ptr, const int32_t* bag_items, int64_t B, int64_t n, int mode,
                 float denom, orx_table* out, int64_t out_row0, int flags);
int orx_seqrec_step(orx_ctx* ctx, int loss_kind /* orx_multineg_kind */, orx_opt* opt,
                    orx_table* hist, orx_table* item, orx_table* bias /* NULL ok */,
                    const int32_t* bag_ptr, const int32_t* bag_items, const int32_t* pid /* [B] */, const int32_t* nid /* [B][N] */,
                    const float* weight /* NULL ok */, const float* neg_offset /* NULL ok */,
                    int64_t B, int64_t n, int32_t N, int mode, float denom, float l2_reg, int train_mask, int flags,
                    float* loss_out, float* l2_out);
int orx_seqrec_loss(orx_ctx* ctx, int loss_kind /* orx_multineg_kind */,
                    orx_table* hist, orx_table* item, orx_table* bias /* NULL ok */,
                    const int32_t* bag_ptr, const int32_t* bag_items, const int32_t* pid /* [B] */, const int32_t* nid /* [B][N] */,
                    const float* weight /* NULL ok */, const float* neg_offset /* NULL ok */,
                    int64_t B, int64_t n, int32_t N, int mode, float denom, int flags, float* loss_out, float* l2_out);

/* ---- THE FULL SOFTMAX OVER ALL ITEMS (api_fullsoftmax.hip, api_seqrec.hip, kernels_fullsoftmax.hip): one train step of a
 * dot-product model under sparse_softmax_cross_entropy over EVERY row of the item table -- the objective of the reference's
 * mlp_softmax / rnn_softmax interactions and of GRU4Rec / SASRec / Mult-VAE style models (a label SET per sample, the
 * multinomial likelihood of Mult-VAE / Mult-DAE: orx_seqrec_full_sets_step, below).  No B x NI matrix is stored.
 * Sample i has a query vector u_i and a label item pid[i].  u_i = U[uid[i]] (orx_fullsoftmax_*: the user-table form) or the
 * pooled q_i of bag i, pooled exactly as orx_bag_pool does (orx_seqrec_full_*: the SeqRec form; hist, item, bias, the bags, mode
 * and denom as in the block above).  The columns are all NI rows of the item table, each once.
 *   s_ij    = scale * (u_i . V[j] + b[j]) + off[j]        j in [0, NI);  no "+ b" with bias == NULL
 *   lse_i   = logsumexp_j s_ij                            evaluated with the maximum subtracted: |s| of 200 stays finite
 *   l_i     = lse_i - s_{i,pid[i]}
 *   loss    = (1/B) sum_i w_i l_i                         w_i = weight[i], 1 when weight == NULL
 *   l2_loss = 1/2 (sum_i |u_i|^2 + sum_i |V[pid[i]]|^2)   the 2B looked-up rows, as orx_inbatch_step: no biases, never weighted
 *   J       = loss + l2_reg * l2_loss
 * scale is finite and > 0.  off = item_offset[NI] is one float per ITEM (a log-prior), 0 when NULL; -inf removes the item from
 * every row's softmax (a padding id, a retired item).  It lives where the ids live and is not validated; a label whose own offset
 * is -inf is the caller's error.  loss_out is the loss, l2_out the UNSCALED l2_loss.
 * Gradients, on the pre-step tables, with c_i = w_i / B, pi_ij = exp(s_ij - lse_i) and n_j = the number of live samples whose
 * label is j:
 *   A_i    = sum over j != pid[i] of pi_ij               (the pi themselves, never 1 - pi_label)
 *   a_ij   = c_i pi_ij  (j != pid[i]),   a_{i,pid[i]} = -c_i A_i
 *   g_u[i] = scale * sum_j a_ij V[j] + l2_reg u_i                       B rows
 *   G_V[j] = scale * sum_i a_ij u_i  + l2_reg n_j V[j]                  ALL NI rows: a dense gradient
 *   G_b[j] = scale * sum_i a_ij
 * The apply.  User side: orx_apply_rows(user, NULL, uid, ...) in the user-table form; orx_seqrec_step's history route in the SeqRec
 * form (occurrence e of bag i has the row c_i * g_q[i]; the n x D occurrence rows never exist).  The item table and the bias take
 * the Keras DENSE rule of the optimizer on every row (as orx_table_apply_dense, as TensorFlow treats a Dense(total_items) kernel).
 * Adam: item and bias are read in full, so lazily applied rows of theirs are finished before the forward and the two leave the
 * lazy set; the user / history table stays lazy, and exactly the rows read are touched; the counter advances once per step,
 * after the reads and before the applies.  One step per call.  loss_out == l2_out == NULL with ORX_IDS_DEVICE: no host
 * synchronisation.  train_mask: ORX_TRAIN_USER (the user / history table) | _ITEM | _BIAS, 0 = every table given; a table outside
 * the mask is read and never written, its optimizer slots are untouched; with neither item nor bias in the mask the item-side
 * gradient pass is not launched.
 * No float atomics anywhere: every sum has a fixed order that depends on (B, NI, D) and the chunking alone, so loss_out, l2_out,
 * the row losses and all tables are bit-repeatable from run to run.  The forward-only calls give the step's loss_out / l2_out
 * bit for bit and, if row_loss_out is not NULL, l_i of every sample ([B], where the ids live; 0 for a dropped sample).
 * chunk_items / chunk_samples: items per chunk of the walks that own samples / samples per chunk of the walk that owns items; 0 --
 * the launcher's own choice, a function of (B, NI, D) alone -- or a positive multiple of the tile width 64.
 * flags: ORX_IDS_DEVICE, ORX_NO_L2 (the steps).  B == 0: ORX_OK, nothing is launched.
 * ORX_ERR_ARG before any device work: what orx_inbatch_step and orx_seqrec_step refuse for the same arguments (dims unequal or
 * above 256; a bias that is not [NI, 1]; scale; l2_reg; ORX_NO_L2 with l2_reg != 0; ORX_HOGWILD, ORX_CENSOR; another context; a
 * bad host bag_ptr; hist == item; what orx_apply_rows refuses); a chunk argument that is negative or no multiple of 64, or so
 * small that a walk would have more than 65535 chunks; B or NI outside 31 bits; a train mask with unknown bits, or
 * ORX_TRAIN_BIAS without a bias.
 * An id outside its table (uid, pid, an id in a bag) or a malformed device bag_ptr: ORX_ERR_INDEX, reported as orx_inbatch_step /
 * orx_seqrec_step report it.  The id is never an address; its sample has c_i = 0 and contributes no loss, no l2, no gradient and
 * no n_j; the context stays usable.
 *   orx_fullsoftmax_geometry   no device: out = { own rows per workgroup, rows per tile, item chunks, sample chunks, padded dim,
 *                              scratch bytes of a step of the user-table form with every table trained }
 * Not offered: dropout between the query and the item table (hidden layers: orx_tower_step, below); K-step calls; UCML / L2 scoring; hit masking (every
 * item is one column); a sampled or sharded item axis; label sets in the user-table form (orx_seqrec_full_sets_step and
 * orx_tower_sets_step have them). */
int orx_fullsoftmax_step(orx_ctx* ctx, orx_opt* opt,
                         orx_table* user, orx_table* item, orx_table* bias /* NULL ok */,
                         const int32_t* uid, const int32_t* pid,
                         const float* weight /* NULL ok */, const float* item_offset /* [NI], NULL ok */,
                         int64_t B, float scale, float l2_reg, int32_t chunk_items, int32_t chunk_samples, int train_mask, int flags,
                         float* loss_out, float* l2_out);
int orx_fullsoftmax_loss(orx_ctx* ctx,
                         orx_table* user, orx_table* item, orx_table* bias /* NULL ok */,
                         const int32_t* uid, const int32_t* pid,
                         const float* weight /* NULL ok */, const float* item_offset /* [NI], NULL ok */,
                         int64_t B, float scale, int32_t chunk_items, int flags,
                         float* loss_out, float* l2_out, float* row_loss_out /* NULL ok */);
int orx_fullsoftmax_geometry(int64_t B, int64_t NI, int32_t D, int32_t chunk_items, int32_t chunk_samples, int64_t out[6]);
int orx_seqrec_full_step(orx_ctx* ctx, orx_opt* opt,
                         orx_table* hist, orx_table* item, orx_table* bias /* NULL ok */,
                         const int32_t* bag_ptr, const int32_t* bag_items, const int32_t* pid /* [B] */,
                         const float* weight /* NULL ok */, const float* item_offset /* [NI], NULL ok */,
                         int64_t B, int64_t n, int mode, float denom, float scale, float l2_reg,
                         int32_t chunk_items, int32_t chunk_samples, int train_mask, int flags, float* loss_out, float* l2_out);
int orx_seqrec_full_loss(orx_ctx* ctx,
                         orx_table* hist, orx_table* item, orx_table* bias /* NULL ok */,
                         const int32_t* bag_ptr, const int32_t* bag_items, const int32_t* pid /* [B] */,
                         const float* weight /* NULL ok */, const float* item_offset /* [NI], NULL ok */,
                         int64_t B, int64_t n, int mode, float denom, float scale, int32_t chunk_items, int flags,
                         float* loss_out, float* l2_out, float* row_loss_out /* NULL ok */);

/* ---- THE HISTORY-POOLED RECOMMENDER WITH A DENSE TOWER (api_tower.hip, kernels_tower.hip): the reference's YouTubeRec /
 * VanillaYouTubeRec -- user-feature embeddings beside the pooled history, hidden layers, the softmax over all items.  Sample i:
 *   x0_i    = [ S_1[f_1[i]] | ... | S_m[f_m[i]] | pool(H[bag_i]) ]         the side rows first, then the pool of orx_bag_pool (its bits)
 *   x_{l+1} = act_l(x_l W_l + c_l),  l = 0 .. L-1                          act = relu (relu'(0) = 0); the last layer's only if relu_last
 *   q_i     = x_L;  s_ij, lse_i, l_i and loss as orx_seqrec_full_step has them on q_i
 *   l2_loss = 1/2 (sum_i |x0_i|^2 + sum_i |V[pid[i]]|^2)                   on the embedding outputs; the layers' part is not in l2_out
 *   J       = loss + l2_reg * l2_loss + l2_mlp * 1/2 sum_l (|W_l|^2 + |c_l|^2)
 * hist [items, Dh]; item [items, Dq], bias [items, 1] or NULL; side[j] [n_j, d_j], n_side in 0 .. 4, side_ids[j] an id list [B]
 * that lives where the bags live; W[l] [in_l, out_l] and c[l] [1, out_l] (c NULL, or an entry NULL: no bias), n_layers in 1 .. 4,
 * in_0 = sum d_j + Dh, in_{l+1} = out_l, out_{L-1} = Dq; every width, in_0 included, in 1 .. 256.  bags, mode, denom, pid, weight,
 * item_offset, scale and the chunk arguments as in orx_seqrec_full_step.
 * An EMPTY bag pools to zeros and stays a live sample (as in orx_seqrec_full_step, where its query is then 0): here its query comes
 * from the side rows and the biases, and the layers take its gradient.  A sample with a bad id -- in its bag or in a side list --
 * is dropped as a whole (x0 = 0, no loss, no l2, no gradient) and the call reports ORX_ERR_INDEX as orx_seqrec_full_step does.
 * The step's order: every check; the lists staged; the lazy rows of every side table and of hist touched; item, bias and every
 * layer finished and out of the lazy set; input, tower forward, full-softmax forward and gradients, tower backward (one pass over
 * g_{l+1} per layer: g_l, and per-batch-chunk partials of dW_l and dc_l), one finishing launch; the Adam counter once; the applies:
 * hist by the sorted route (occurrence e of bag i takes c_i * g_0[i][sum d_j ..]), side[j] by orx_apply_rows with side_ids[j]
 * (rows outside the batch stay as they are), item, bias, W_l and c_l by the optimizer's dense rule.  No float atomics: all results
 * are bit-repeatable; a row of the tower's output has the same bits in any batch.
 * train_mask: ORX_TRAIN_USER (hist) | _ITEM | _BIAS | ORX_TRAIN_SIDE (every side table) | ORX_TRAIN_TOWER (every W_l and c_l);
 * 0 = every table given.  flags: ORX_IDS_DEVICE, ORX_NO_L2 (then l2_reg == l2_mlp == 0).
 * ORX_ERR_ARG before any device work, beyond what orx_seqrec_full_step refuses: n_layers outside 1 .. 4, n_side outside 0 .. 4; a
 * width outside 1 .. 256; a layer whose inputs do not chain, a last layer that is not the item table's dim wide; c_l not
 * [1, out_l]; a table passed twice; l2_mlp negative or not finite; ORX_TRAIN_SIDE without a side table; an optimizer that
 * orx_apply_rows refuses for hist or a side table.
 *   orx_tower_loss       forward only: the step's loss_out / l2_out bit for bit, and l_i per sample if row_loss_out is not NULL
 *   orx_tower_query      q_i of B bags into rows [out_row0, out_row0 + B) of `out` [.., out_{L-1}]: the queries the step uses, bit for bit
 *   orx_tower_geometry   no device: out = { rows per tile, batch chunks of the backward, tiles per chunk, scratch bytes of a step with
 *                        every table trained beyond the lists' and the full softmax's } for B samples and widths[n_layers + 1]
 * Not offered: the sampled-negatives form (orx_seqrec_step with a tower), dropout, batch norm, K-step calls. */
enum orx_tower_train_mask { ORX_TRAIN_SIDE = 16, ORX_TRAIN_TOWER = 32 };      /* beside orx_train_mask's three (8 is ORX_TRAIN_PROJ) */
int orx_tower_step(orx_ctx* ctx, orx_opt* opt,
                   orx_table* hist, orx_table* item, orx_table* bias /* NULL ok */,
                   int32_t n_side, orx_table* const* side, const int32_t* const* side_ids,
                   int32_t n_layers, orx_table* const* W, orx_table* const* c /* NULL ok */, int relu_last,
                   const int32_t* bag_ptr, const int32_t* bag_items, const int32_t* pid /* [B] */,
                   const float* weight /* NULL ok */, const float* item_offset /* [NI], NULL ok */,
                   int64_t B, int64_t n, int mode, float denom, float scale, float l2_reg, float l2_mlp,
                   int32_t chunk_items, int32_t chunk_samples, int train_mask, int flags, float* loss_out, float* l2_out);
int orx_tower_loss(orx_ctx* ctx,
                   orx_table* hist, orx_table* item, orx_table* bias /* NULL ok */,
                   int32_t n_side, orx_table* const* side, const int32_t* const* side_ids,
                   int32_t n_layers, orx_table* const* W, orx_table* const* c /* NULL ok */, int relu_last,
                   const int32_t* bag_ptr, const int32_t* bag_items, const int32_t* pid /* [B] */,
                   const float* weight /* NULL ok */, const float* item_offset /* [NI], NULL ok */,
                   int64_t B, int64_t n, int mode, float denom, float scale, int32_t chunk_items, int flags,
                   float* loss_out, float* l2_out, float* row_loss_out /* NULL ok */);
int orx_tower_query(orx_ctx* ctx, orx_table* hist,
                    int32_t n_side, orx_table* const* side, const int32_t* const* side_ids,
                    int32_t n_layers, orx_table* const* W, orx_table* const* c /* NULL ok */, int relu_last,
                    const int32_t* bag_ptr, const int32_t* bag_items, int64_t B, int64_t n, int mode, float denom,
                    orx_table* out, int64_t out_row0, int flags);
int orx_tower_geometry(int64_t B, int32_t n_layers, const int32_t* widths /* [n_layers + 1] */, int64_t out[4]);

/* ---- LABEL SETS UNDER THE FULL SOFTMAX (api_fullsoftmax.hip, api_seqrec.hip, api_tower.hip, kernels_labelsets.hip): the
 * multinomial likelihood of Mult-DAE / Mult-VAE (Liang et al. 2018) -- a sample's query against every item, scored on the
 * sample's WHOLE SET of items in one walk.  orx_seqrec_full_sets_* and orx_tower_sets_* are orx_seqrec_full_* and orx_tower_*
 * with pid replaced by ragged label lists.  Sample i has the query q_i of its form (the pooled history; the tower's output)
 * and the entries e in [lab_ptr[i], lab_ptr[i + 1]), each an item j_e = lab_items[e] with a weight t_e = lab_weight[e], 1 when
 * lab_weight == NULL.  A duplicate in a set is two entries.  T_i = sum_e t_e.  s_ij, lse_i, scale, item_offset, weight,
 * c_i = w_i / B and pi_ij as in orx_seqrec_full_step.
 *   l_i     = T_i lse_i - sum_e t_e s_{i,j_e}
 *   loss    = (1/B) sum_i w_i l_i
 *   l2_loss = 1/2 (sum_i |the query side's rows as in the single-label call|^2 + sum over live entries e of |V[j_e]|^2)
 *   a_ij    = c_i (T_i pi_ij - sum over e of set i with j_e = j of t_e)
 *   g_q[i]  = scale * sum_j a_ij V[j] + (the single-label call's l2 term)
 *   G_V[j]  = scale * sum_i a_ij q_i  + l2_reg n_j V[j]       n_j = the number of live label entries with item j, not weighted by t
 *   G_b[j]  = scale * sum_i a_ij
 * An EMPTY set: the sample stays live with T_i = 0; it contributes its query side's l2 part and nothing else.  Sets of one with
 * t = 1 are the single-label objective, equal to fp32 rounding and NOT bit for bit: here the label is one of the items summed
 * into the softmax's denominator and its coefficient is formed by a subtraction on the finished gradient, where the
 * single-label walks keep the label out of the sum.  The single-label calls' results are unchanged in every bit.
 * An id outside the item table in a label set, a bad id in the bag or in a side list, or a malformed device lab_ptr (negative,
 * decreasing, beyond n_lab, lab_ptr[0] != 0, lab_ptr[B] != n_lab) drops the sample as a whole and reports ORX_ERR_INDEX as the bag
 * lists do; the id is never an address; the context stays usable.  A bad HOST lab_ptr is ORX_ERR_ARG before any device work.
 * lab_weight lives where the ids live and is not validated, like item_offset.
 * The apply rules, the lazy-Adam order, the train masks, the flags, the refusals and B == 0 are the single-label calls'.
 * The dense part c_i T_i pi_ij is the single-label walks on rows no item is the label of; the sparse part: one wavefront per
 * sample over its entries (64 ids per load) for the scores, T_i, sum_e t_e V[j_e] and the |V|^2; the label entries sorted by
 * item (the stable sort of orx_apply_rows) and one wavefront per run of equal items, in position order, for G_V, G_b and n_j.
 * No float atomics: every sum has a fixed order that depends on the lists and the shapes alone; losses, row losses and all tables
 * are bit-repeatable from run to run.  The forward-only calls give the step's loss_out / l2_out bit for bit.
 * Not offered: label sets in the user-table form (orx_fullsoftmax_step); the VAE's sampling and KL term; tanh; a 1 / sqrt(len)
 * pool; dropout inside the tower; the sampled-negatives form with sets; K-step calls. */
int orx_seqrec_full_sets_step(orx_ctx* ctx, orx_opt* opt,
                              orx_table* hist, orx_table* item, orx_table* bias /* NULL ok */,
                              const int32_t* bag_ptr, const int32_t* bag_items,
                              const int32_t* lab_ptr /* [B + 1] */, const int32_t* lab_items /* [n_lab] */,
                              const float* lab_weight /* [n_lab], NULL ok */, int64_t n_lab,
                              const float* weight /* NULL ok */, const float* item_offset /* [NI], NULL ok */,
                              int64_t B, int64_t n, int mode, float denom, float scale, float l2_reg,
                              int32_t chunk_items, int32_t chunk_samples, int train_mask, int flags, float* loss_out, float* l2_out);
int orx_seqrec_full_sets_loss(orx_ctx* ctx,
                              orx_table* hist, orx_table* item, orx_table* bias /* NULL ok */,
                              const int32_t* bag_ptr, const int32_t* bag_items,
                              const int32_t* lab_ptr /* [B + 1] */, const int32_t* lab_items /* [n_lab] */,
                              const float* lab_weight /* [n_lab], NULL ok */, int64_t n_lab,
                              const float* weight /* NULL ok */, const float* item_offset /* [NI], NULL ok */,
                              int64_t B, int64_t n, int mode, float denom, float scale, int32_t chunk_items, int flags,
                              float* loss_out, float* l2_out, float* row_loss_out /* NULL ok */);
int orx_tower_sets_step(orx_ctx* ctx, orx_opt* opt,
                        orx_table* hist, orx_table* item, orx_table* bias /* NULL ok */,
                        int32_t n_side, orx_table* const* side, const int32_t* const* side_ids,
                        int32_t n_layers, orx_table* const* W, orx_table* const* c /* NULL ok */, int relu_last,
                        const int32_t* bag_ptr, const int32_t* bag_items,
                        const int32_t* lab_ptr /* [B + 1] */, const int32_t* lab_items /* [n_lab] */,
                        const float* lab_weight /* [n_lab], NULL ok */, int64_t n_lab,
                        const float* weight /* NULL ok */, const float* item_offset /* [NI], NULL ok */,
                        int64_t B, int64_t n, int mode, float denom, float scale, float l2_reg, float l2_mlp,
                        int32_t chunk_items, int32_t chunk_samples, int train_mask, int flags, float* loss_out, float* l2_out);
int orx_tower_sets_loss(orx_ctx* ctx,
                        orx_table* hist, orx_table* item, orx_table* bias /* NULL ok */,
                        int32_t n_side, orx_table* const* side, const int32_t* const* side_ids,
                        int32_t n_layers, orx_table* const* W, orx_table* const* c /* NULL ok */, int relu_last,
                        const int32_t* bag_ptr, const int32_t* bag_items,
                        const int32_t* lab_ptr /* [B + 1] */, const int32_t* lab_items /* [n_lab] */,
                        const float* lab_weight /* [n_lab], NULL ok */, int64_t n_lab,
                        const float* weight /* NULL ok */, const float* item_offset /* [NI], NULL ok */,
                        int64_t B, int64_t n, int mode, float denom, float scale, int32_t chunk_items, int flags,
                        float* loss_out, float* l2_out, float* row_loss_out /* NULL ok */);

/* Diagnostics of the duplicate plan of the exact steps (api_plan.hip; DESIGN.md "The duplicate plan as tested").
 *   orx_plan_geometry   host only, no device: out[16] = {nru, nri, lgu, lgi, shift, W (32-bit words per range bitmap), PL_UN, PL_LCNT,
 *                       PL_PAIR_CAP, ORX_SEG_DIRECT, ORX_PIECE, threads per range workgroup, threads of a big plan, references per
 *                       partition workgroup, rows per range of the first plan (dedup_kernel), its user ranges} for tables of NU / NI rows
 *                       and nU / nP / nN references per step
 *   orx_plan_dump       the plan of K steps of B triplets (nid NULL: samples, `label` optional) for tables of NU / NI rows and dim D, made
 *                       on the route the train steps take; ids and labels are HOST arrays [K][B].
 *                       opts[8] = {plan version (1: dedup_kernel + urgent_kernel, 2: bucketed; must be the one the process runs, ORX_PLAN_V1),
 *                                  staging, urgent marks, pairing tpw (0: off, else orx_fused_tpw(D)), min_late (-1: heuristic),
 *                                  force 1024-thread workgroups, step0 (> 0: planned as [0, step0) then [step0, K)), 0}
 *                       out[10] = host buffers (each may be NULL), per step, padding removed: rewritten ids int32 [K][3][B]; pairing words
 *                                  int32 [K][B] (origin << 10 | ORX_PAIR bits); dlist uint32 [K][2B]; dcount [K]; alloc [K][8];
 *                                  refinfo [K][3][B][2]; segstart [K][B]; dseg [K][2B]; dcnt [K][2B]; tree items [K][item_stride][4]
 *                       info[8] = {item_stride, tree_off[3], index-error flag of the context (read only: it stays for orx_check_index_error),
 *                                  1024-thread workgroups chosen for the NEXT plan, Bp, steps per chunk}
 *                       out == NULL: sizes the buffers and fills info only.  Synchronizes the stream. */
int orx_plan_geometry(int64_t NU, int64_t NI, int64_t nU, int64_t nP, int64_t nN, int32_t* out);
int orx_plan_dump(orx_ctx* ctx, const int32_t* uid, const int32_t* pid, const int32_t* nid, const float* label, int64_t K, int64_t B,
                  int64_t NU, int64_t NI, int32_t D, const int32_t* opts, void* const* out, int64_t* info);

#ifdef __cplusplus
}
#endif
#endif /* OPENREC_HIP_H */
