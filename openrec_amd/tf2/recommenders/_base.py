"""Shared machinery of the recommenders: a model call either runs the
forward-only kernel (no tape) or records a pending fused step (under a tape,
see openrec_amd/tf2/_lazy.py)."""
from __future__ import annotations

import os

import numpy as np

from ... import runtime as rt
from .._lazy import LazyScalar, PendingStep, active_tape

# consecutive applied steps wait in a queue of this many and run as ONE K-step device call (0: no queue)
STEP_QUEUE = int(os.environ.get("ORX_STEP_QUEUE", "32"))


class _StepQueue:
    """Snapshot of the inputs of up to STEP_QUEUE applied-but-not-yet-executed train steps of one model."""

    def __init__(self):
        self.steps, self.key, self.bufs, self.runner, self.censor = [], None, None, None, []
        self.subset = False

    def add(self, step, key, arrays, runner, subset=False):
        """arrays: the per-step input arrays (all of one length B); runner(bufs, K) -> (loss[K], l2[K]); subset: the queued
        steps train a strict subset of the model's tables (part of `key`: such steps never share a call with others)"""
        cap = STEP_QUEUE
        if self.bufs is None:
            self.key, self.runner, self.subset = key, runner, subset
            self.bufs = []
            for a in arrays:
                if hasattr(a, "is_cuda") and a.is_cuda:
                    import torch
                    self.bufs.append(torch.empty((cap,) + tuple(a.shape), dtype=a.dtype, device=a.device))
                else:
                    a = np.asarray(a)
                    self.bufs.append(np.empty((cap,) + a.shape, a.dtype))
        k = len(self.steps)
        for buf, a in zip(self.bufs, arrays):
            if isinstance(buf, np.ndarray):
                buf[k] = np.asarray(a)
            else:
                buf[k].copy_(a)
        self.steps.append(step)

    def run(self):
        steps, bufs, runner, flags = self.steps, self.bufs, self.runner, self.censor
        self.steps, self.key, self.bufs, self.runner, self.censor = [], None, None, None, []
        K = len(steps)
        if K == 0:
            return
        flags = flags + [False] * (K - len(flags))
        k0 = 0
        while k0 < K:                               # consecutive steps with the same censor flag share a device call
            k1 = k0
            while k1 < K and flags[k1] == flags[k0]:
                k1 += 1
            kw = {"censor": True} if flags[k0] else {}
            loss, l2 = runner([b[k0:k1] for b in bufs], k1 - k0, **kw)
            for i in range(k0, k1):
                steps[i].values = (float(loss[i - k0]), float(l2[i - k0]))
                steps[i].trained, steps[i].queued = True, False
            k0 = k1

    def mark_censor(self, arrays):
        """UCML.censor_vec right after a queued step with the same ids: fold it into that step (ORX_CENSOR)."""
        k = len(self.steps) - 1
        if k < 0 or len(self.censor) > k or self.subset:      # (a subset step takes no folded censor: it runs as its own call)
            return False
        for buf, a in zip(self.bufs, arrays):
            if isinstance(buf, np.ndarray):
                if hasattr(a, "is_cuda") or not np.array_equal(buf[k], np.asarray(a)):
                    return False
            else:
                if not (hasattr(a, "is_cuda") and a.is_cuda and bool((buf[k] == a).all())):
                    return False
        self.censor = self.censor + [False] * (k - len(self.censor)) + [True]
        return True


def _ids(x):
    if hasattr(x, "numpy") and not isinstance(x, np.ndarray) and not getattr(x, "is_cuda", False):
        x = x.numpy()
    return x


class Recommender:
    """Base of BPR / UCML / GMF / WRMF: three tables exactly as in the reference
    constructors (user_latent_factor, item_latent_factor, item_bias); `item_bias` is None in a model built
    without item biases (BPR(use_item_bias=False))."""

    def _build_tables(self, dim_user_embed, dim_item_embed, total_users, total_items, ctx=None, item_bias=True):
        from ..modules import LatentFactor
        if dim_user_embed != dim_item_embed:
            # the reference multiplies / subtracts the two vectors element-wise, so unequal
            # dims fail inside TF at the first call; fail at construction instead
            raise ValueError("dim_user_embed and dim_item_embed must be equal")
        self.user_latent_factor = LatentFactor(num_instances=total_users, dim=dim_user_embed,
                                               name='user_latent_factor', ctx=ctx)
        self.item_latent_factor = LatentFactor(num_instances=total_items, dim=dim_item_embed,
                                               name='item_latent_factor', ctx=ctx)
        self.item_bias = LatentFactor(num_instances=total_items, dim=1, name='item_bias', ctx=ctx) if item_bias else None
        self._queue = _StepQueue()
        for lf in self._factors():
            lf.table.pre_access = self.flush          # any host-visible access to a table first runs the queued steps

    def _factors(self):
        """the model's LatentFactor modules (item_bias left out where the model has none)"""
        return [lf for lf in (self.user_latent_factor, self.item_latent_factor, self.item_bias) if lf is not None]

    def flush(self):
        """Run the queued train steps now (called automatically whenever their effect could be observed)."""
        if getattr(self, "_queue", None) is not None:
            self._queue.run()

    def _enqueue(self, step, key, arrays, runner, subset=False):
        """Queue an applied step; returns False when queuing is off (the caller then runs it directly)."""
        if STEP_QUEUE <= 1:
            return False
        q = self._queue
        if q.steps and q.key != key:
            q.run()
        q.add(step, key, arrays, runner, subset)
        if len(q.steps) >= STEP_QUEUE:
            q.run()
        return True

    @property
    def trainable_variables(self):
        """the variables of the LatentFactors whose `trainable` is set (Keras: `layer.trainable = False` freezes a table)"""
        return [v for lf in self._factors() for v in lf.trainable_variables]

    @property
    def variables(self):
        return [v for lf in self._factors() for v in lf.variables]

    def _train_roles(self, variables):
        """The variables handed to apply_gradients for a step of this model -> None (all of them: the full step) or the
        roles ("user" / "item" / "bias") of a strict subset, by table identity."""
        roles = {"user": self.user_latent_factor, "item": self.item_latent_factor, "bias": self.item_bias}
        tables = {name: lf.table for name, lf in roles.items() if lf is not None}
        mlp = getattr(self, "mlp", None)                     # GMF: the Dense(1) kernel is a variable of the step too
        extra = list(mlp.trainable_variables) if mlp is not None else []
        got, got_extra = [], []
        for v in variables:
            t = getattr(v, "table", None)
            name = next((n for n, tt in tables.items() if t is tt), None)
            k = next((i for i, e in enumerate(extra) if t is e.table), None)
            if name is not None:
                if name not in got:
                    got.append(name)
            elif k is not None:
                if k not in got_extra:
                    got_extra.append(k)
            else:
                raise ValueError(f"apply_gradients: variable {getattr(v, 'name', None) or v!r} does not belong to the model of its "
                                 f"gradient's step ({type(self).__name__})")
        if len(got) == len(tables) and len(got_extra) == len(extra):
            return None
        if extra:
            missing = [roles[n]._var.name for n in tables if n not in got] + [e.name for i, e in enumerate(extra) if i not in got_extra]
            raise NotImplementedError(f"{type(self).__name__} (GMF): training a strict subset of the variables is not supported (the Dense "
                                      f"kernel is a fourth role); apply_gradients was not handed {missing}")
        return tuple(n for n in ("user", "item", "bias") if n in got)

    def _tables(self, flush=True):
        if flush:
            self.flush()
        return (self.user_latent_factor.table, self.item_latent_factor.table,
                self.item_bias.table if self.item_bias is not None else None)

    _score_kind = "dot"

    def evaluate(self, user_id, pos_mask, excl_mask=None, at=(100,), score_matrix=True, cand_mask=None):
        """Beyond the reference API: `eval_step` of tf2_examples/bpr_citeulike.py:41-46 as one device call
        (all-item scores + AUC / NDCG / Recall; the [B, n_items] score matrix never reaches the host).  The masks as
        `Dataset.evaluation` yields them (item lists, `rt.SparseMask`) go over as lists; dense masks are accepted too
        (both as lists when they are sparse enough to be worth the host-side nonzero).  `score_matrix=False`: the same numbers
        bit for bit from `rt.rank_metrics_matrixfree`, whose device scratch does not grow with users x items (dense masks
        go through `SparseMask.from_dense`).  `cand_mask` instead of `excl_mask` (what `Dataset.evaluation(candidates=True)`
        yields): the universe of each user is its candidate list, the numbers are those of `excl_mask = ~cand_mask` bit for
        bit, and only the listed items are scored (`rt.rank_metrics_candidates`)."""
        if cand_mask is not None and excl_mask is not None:
            raise ValueError("evaluate takes excl_mask or cand_mask, not both")
        if cand_mask is None and excl_mask is None:
            raise ValueError("evaluate needs excl_mask or cand_mask")
        U, V, b = self._tables()
        w = self.mlp.layers[0].kernel if self._score_kind == "gmf" else None
        kw = dict(kind=self._score_kind, user=U, item=V, bias=b, w=w, uid=_ids(user_id))
        if cand_mask is not None:
            pos, cand = (m if isinstance(m, rt.SparseMask) else rt.SparseMask.from_dense(m) for m in (pos_mask, cand_mask))
            return rt.rank_metrics_candidates(pos, cand, list(at), **kw)
        if not score_matrix:
            pos, excl = (m if isinstance(m, rt.SparseMask) else rt.SparseMask.from_dense(m) for m in (pos_mask, excl_mask))
            return rt.rank_metrics_matrixfree(pos, excl, list(at), **kw)
        if isinstance(pos_mask, rt.SparseMask) and isinstance(excl_mask, rt.SparseMask):
            return rt.rank_metrics_csr(pos_mask, excl_mask, list(at), **kw)
        return rt.rank_metrics(pos_mask, excl_mask, list(at), **kw)

    def recommend(self, user_id, k, excl_mask=None):
        """Beyond the reference API: the k best items of each user as (item ids [B, k], scores [B, k]) in one device call,
        without the [B, n_items] score matrix of `inference`.  Scores equal `inference`'s bit for bit, ordered by score
        descending and then item id ascending; items in `excl_mask` (as `Dataset.evaluation` yields it, `rt.SparseMask`, or a
        dense bool mask) and NaN scores are never returned, and rows with fewer than k other items end in id -1 / -inf."""
        U, V, b = self._tables()
        w = self.mlp.layers[0].kernel if self._score_kind == "gmf" else None
        return rt.recommend_topk(self._score_kind, U, V, b, _ids(user_id), k, excl=excl_mask, w=w)

    def score(self, user_id, candidates):
        """Beyond the reference API: the scores of each user's own candidate list (the re-ranking stage after `recommend` or
        any other retrieval) -> a list of float32 arrays, one per user, aligned with its candidates.  `candidates`: one id
        array per user, in any order and with repeats (or an `rt.SparseMask` / `rt.CandidateLists`).  Scores equal
        `inference`'s at the same places bit for bit; only the listed items are scored."""
        U, V, b = self._tables()
        w = self.mlp.layers[0].kernel if self._score_kind == "gmf" else None
        cand = rt.as_candidate_lists(candidates, V.rows)
        flat = rt.score_candidates(self._score_kind, U, V, b, _ids(user_id), cand, w=w)
        return [flat[cand.ptr[q]:cand.ptr[q + 1]] for q in range(cand.shape[0])]

    def _record(self, run_forward, run_train):
        for lf in self._factors():
            lf.snapshot_pending()               # lookups made before this step see the rows as they are now (TF gathers at call time)
        step = PendingStep(self, run_forward, run_train)
        tape = active_tape()
        if tape is not None:
            tape.record(step)
        else:
            step.forward()                      # eager semantics outside a tape
        # the call returns (loss, l2_reg * l2_loss): a tape over the tuple trains loss + l2_reg * l2_loss (TF sums a nested target)
        return LazyScalar(step, 0), LazyScalar(step, 1, scale=self.l2_reg)

    l2_reg = 1.0                                # the reference's objective (bpr_citeulike.py:36-37)

    def _set_l2_reg(self, l2_reg):
        l2_reg = float(l2_reg)
        if not (np.isfinite(l2_reg) and l2_reg >= 0):
            raise ValueError(f"l2_reg must be finite and >= 0, got {l2_reg!r}")
        self.l2_reg = l2_reg

    def _l2_arg(self, no_l2):
        """rt.*_step's l2_reg for a step of this model: None (today's entry points) for the reference's weight 1 and for no_l2"""
        return None if (no_l2 or self.l2_reg == 1.0) else self.l2_reg


class PointwiseRecommender(Recommender):
    """GMF / WRMF: (user, item, label) samples; `_point_args()` gives (model name, dense kernel table or None, kwargs)."""

    def __call__(self, user_id, item_id, label):
        tape = active_tape()
        U, V, b = self._tables(flush=tape is None)
        name, w, kw = self._point_args()
        uid, iid, lab = _ids(user_id), _ids(item_id), _ids(label)
        step_holder = []

        def run_forward():
            self.flush()
            return rt.pointwise_loss(name, U, V, b, w, uid, iid, lab, **kw)

        def run_train(optimizer, no_l2, train=None):
            def runner(bufs, K):
                return rt.pointwise_step(name, optimizer, U, V, b, w, bufs[0], bufs[1], bufs[2], K=K, no_l2=no_l2, train=train,
                                         l2_reg=l2_reg, **kw)
            l2_reg = self._l2_arg(no_l2)
            n = uid.numel() if hasattr(uid, "numel") else np.asarray(uid).size
            key = ("point", id(optimizer), bool(no_l2), int(n), bool(getattr(uid, "is_cuda", False)), train, l2_reg)
            if self._enqueue(step_holder[0], key, (uid, iid, np.asarray(lab, np.float32) if not hasattr(lab, "is_cuda") else lab), runner,
                             subset=train is not None):
                return None
            loss, l2 = runner((uid, iid, lab), 1)
            return float(loss[0]), float(l2[0])

        out = self._record(run_forward, run_train)
        step_holder.append(out[0]._step)
        return out

    call = __call__


class PairwiseRecommender(Recommender):
    _model = None
    margin = 0.5

    def __call__(self, user_id, p_item_id, n_item_id, sample_weight=None):
        """sample_weight: one weight per triplet (a float array or device tensor living where the ids live); it multiplies the
        triplet's term inside BPR's mean / UCML's sum (rt.pairwise_step's weights)"""
        tape = active_tape()
        U, V, b = self._tables(flush=tape is None)        # under a tape nothing is observed yet: keep the queue
        uid, pid, nid = _ids(user_id), _ids(p_item_id), _ids(n_item_id)
        wts = None
        if sample_weight is not None:
            wts = _ids(sample_weight)
            if not hasattr(wts, "is_cuda"):
                wts = np.ascontiguousarray(wts, np.float32)
        step_holder = []

        def run_forward():
            self.flush()
            return rt.pairwise_loss(self._model, U, V, b, uid, pid, nid, margin=self.margin, weights=wts)

        def run_train(optimizer, no_l2, train=None):
            def runner(bufs, K, censor=False):
                # (both None: today's entry points; the weights are the queue's fourth buffer)
                return rt.pairwise_step(self._model, optimizer, U, V, b, bufs[0], bufs[1], bufs[2], K=K,
                                        margin=self.margin, no_l2=no_l2, censor=censor, train=train,
                                        weights=bufs[3] if wts is not None else None, l2_reg=l2_reg)
            l2_reg = self._l2_arg(no_l2)
            n = uid.numel() if hasattr(uid, "numel") else np.asarray(uid).size
            # a weighted and an unweighted step, or steps of two coefficients, never share a device call
            key = ("pair", id(optimizer), bool(no_l2), int(n), bool(getattr(uid, "is_cuda", False)), self.margin, train,
                   l2_reg, wts is not None)
            arrays = (uid, pid, nid) if wts is None else (uid, pid, nid, wts)
            if self._enqueue(step_holder[0], key, arrays, runner, subset=train is not None):
                return None
            loss, l2 = runner(arrays, 1)
            return float(loss[0]), float(l2[0])

        out = self._record(run_forward, run_train)
        step_holder.append(out[0]._step)
        return out

    call = __call__

    def train_steps(self, optimizer, user_id, p_item_id, n_item_id, K=None, want_loss=True, censor=False, train=None,
                    sample_weight=None):
        """Beyond the reference API: K consecutive fused steps in one device call
        (ids shaped [K, B]); the path `bench.py` measures.  train: None, or the tables to update ("user", "item",
        "bias") while the others stay as they are (rt.pairwise_step).  sample_weight: per-triplet weights shaped like the
        ids.  The objective is loss + l2_reg * l2_loss with the model's l2_reg; the returned l2 is the unscaled l2_loss."""
        U, V, b = self._tables()
        uid, pid, nid = _ids(user_id), _ids(p_item_id), _ids(n_item_id)
        if K is None:
            K = uid.shape[0] if getattr(uid, "ndim", 1) == 2 else 1
        opt = optimizer.native(U.ctx) if hasattr(optimizer, "native") else optimizer
        wts = _ids(sample_weight) if sample_weight is not None else None
        return rt.pairwise_step(self._model, opt, U, V, b, uid, pid, nid, K=K, margin=self.margin,
                                want_loss=want_loss, censor=censor, train=train, weights=wts, l2_reg=self._l2_arg(False))

    def train_steps_multi(self, optimizer, user_id, p_item_id, n_item_ids, loss="softmax", K=None, want_loss=True,
                          sample_weight=None, neg_offset=None):
        """Beyond the reference API: K consecutive steps of ONE positive against N negatives per sample in one device call
        (rt.multineg_step).  user_id / p_item_id shaped [K, B] (or [B]: one step), n_item_ids [K, B, N] (or [B, N]).
        loss: "softmax" (sampled softmax over the 1 + N logits) or "logsig" (the mean of N BPR pair terms).  sample_weight:
        per-sample weights shaped like user_id; neg_offset: added to the negatives' logits, shaped like n_item_ids.  The
        objective is loss + l2_reg * l2_loss with the model's l2_reg; the returned l2 is the unscaled l2_loss.  Dot-product
        models only: it goes through no tape, takes no train mask, and UCML raises NotImplementedError."""
        if self._model != "bpr":
            raise NotImplementedError(f"{type(self).__name__}.train_steps_multi: the N-negative step scores by dot products "
                                      "(u.v + b); UCML's squared-distance scores are not supported by it")
        U, V, b = self._tables()
        uid, pid, nid = _ids(user_id), _ids(p_item_id), _ids(n_item_ids)
        if K is None:
            K = uid.shape[0] if getattr(uid, "ndim", 1) == 2 else 1
        opt = optimizer.native(U.ctx) if hasattr(optimizer, "native") else optimizer
        wts = _ids(sample_weight) if sample_weight is not None else None
        off = _ids(neg_offset) if neg_offset is not None else None
        return rt.multineg_step(loss, opt, U, V, b, uid, pid, nid, K=K, weights=wts, neg_offset=off, l2_reg=self.l2_reg,
                                want_loss=want_loss)

    def train_steps_inbatch(self, optimizer, user_id, p_item_id, K=None, want_loss=True, sample_weight=None, item_offset=None,
                            scale=1.0, mask_hits=True):
        """Beyond the reference API: K consecutive steps on in-batch negatives in one device call (rt.inbatch_step): every
        sample's positive against the positives of all samples of its step, under a softmax over the row.  user_id / p_item_id
        shaped [K, B] (or [B]: one step).  sample_weight: per-sample weights; item_offset: added to column j of every row
        (-log Q(item) is the log-Q correction); both shaped like the ids.  scale = 1 / temperature; mask_hits: a column with the
        row's own positive item is no negative.  The objective is loss + l2_reg * l2_loss with the model's l2_reg; the returned
        l2 is the unscaled l2_loss.  Dot-product models only: it goes through no tape, takes no train mask, and UCML raises
        NotImplementedError."""
        if self._model != "bpr":
            raise NotImplementedError(f"{type(self).__name__}.train_steps_inbatch: the in-batch step scores by dot products "
                                      "(u.v + b); UCML's squared-distance scores are not supported by it")
        U, V, b = self._tables()
        uid, pid = _ids(user_id), _ids(p_item_id)
        if K is None:
            K = uid.shape[0] if getattr(uid, "ndim", 1) == 2 else 1
        opt = optimizer.native(U.ctx) if hasattr(optimizer, "native") else optimizer
        wts = _ids(sample_weight) if sample_weight is not None else None
        off = _ids(item_offset) if item_offset is not None else None
        return rt.inbatch_step(opt, U, V, b, uid, pid, K=K, weights=wts, item_offset=off, scale=scale, mask_hits=mask_hits,
                               l2_reg=self.l2_reg, want_loss=want_loss)

    def train_steps_full(self, optimizer, user_id, p_item_id, want_loss=True, sample_weight=None, item_offset=None, scale=1.0,
                         train=None):
        """Beyond the reference API: one step on the softmax over ALL items in one device call (rt.fullsoftmax_step): every
        sample's positive is the label among every row of the item table -- no sampler, no B x items matrix.  user_id /
        p_item_id shaped [B].  sample_weight: per-sample weights shaped like the ids; item_offset [total_items]: added to an
        item's logit in every row (a log-prior; -inf removes the item).  scale = 1 / temperature.  The user table takes the
        sparse rule, the item table and the bias the optimizer's dense rule on every row.  train: None, or a subset of
        ("user", "item", "bias").  The objective is loss + l2_reg * l2_loss with the model's l2_reg; the returned l2 is the
        unscaled l2_loss.  Dot-product models only: it goes through no tape, and UCML raises NotImplementedError."""
        if self._model != "bpr":
            raise NotImplementedError(f"{type(self).__name__}.train_steps_full: the full-softmax step scores by dot products "
                                      "(u.v + b); UCML's squared-distance scores are not supported by it")
        U, V, b = self._tables()
        opt = optimizer.native(U.ctx) if hasattr(optimizer, "native") else optimizer
        wts = _ids(sample_weight) if sample_weight is not None else None
        off = _ids(item_offset) if item_offset is not None else None
        return rt.fullsoftmax_step(opt, U, V, b, _ids(user_id), _ids(p_item_id), weights=wts, item_offset=off, scale=scale,
                                   l2_reg=self.l2_reg, train=train, want_loss=want_loss)
