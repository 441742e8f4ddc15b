"""VanillaYouTubeRec (the reference's tf1/recommenders/vanilla_youtube_rec.py with tf1/modules/interactions/mlp_softmax.py): the
user vector is pooled from the embeddings of the items the user just interacted with, and items are scored by a dot product
plus a bias (rt.SeqRec),
    q = pool(H[seq_item_id[:seq_len]]);   s(q, i) = q . V[i] + b[i].
There is no user table: a history never trained on is served like any other.  Three deviations from the reference:
  * no hidden layer by default -- the reference puts Dense(dim_item_embed) layers (and dropout) between the pooled vector and the
    softmax; the default here is the depth-0 tower, the pooled vector itself meets the item table.  `hidden=[...]` puts
    Dense + bias + relu layers of those widths in between (rt.DeepSeqRec; youtube_rec.py has the reference's YouTubeRec, which
    adds the user-feature embeddings); such a model trains through `train_steps_full` only, and without dropout;
  * `train_steps` trains on a sampled softmax (or the log-sigmoid pair loss) over the label and N negatives the caller draws --
    the default, and the cheap one; the reference's full softmax over all items is `train_steps_full` / `loss_full`;
  * the l2 term sits on the POOLED vector and the looked-up rows of the item table; the reference's l2_reg_embed sits on every
    looked-up row of the sequence embedding.
The default pooling divides by max_seq_len, which is the reference's reduce_mean over the zero-masked padded axis;
pool="mean" divides by the history's own length.  Training goes through `train_steps` (no tape); `inference`, `recommend`,
`score` and `evaluate` take histories where the other recommenders take user ids and run on (pooled rows, V, b) through the base
class's paths."""
import numpy as np

from ._base import Recommender, _ids
from ... import runtime as rt


class VanillaYouTubeRec(Recommender):

    def __init__(self, dim_item_embed, max_seq_len, total_items, l2_reg_embed=None, use_item_bias=True, pool=None, ctx=None,
                 hidden=None, l2_reg_mlp=None):
        """pool: None -- ("fixed", max_seq_len) --, "mean", "sum" or ("fixed", denom); l2_reg_embed: the coefficient of the l2 term
        (None: 0).  hidden: None -- the depth-0 model --, or the widths of 1 .. 4 Dense + bias + relu layers between the pooled
        vector and the item table, whose dim is then the last width; l2_reg_mlp: the coefficient on the layers (None: 0)."""
        self._build("VanillaYouTubeRec", dim_item_embed, max_seq_len, total_items, l2_reg_embed, l2_reg_mlp, use_item_bias, pool, ctx,
                    hidden, ())

    def _build(self, what, dim_item_embed, max_seq_len, total_items, l2_reg_embed, l2_reg_mlp, use_item_bias, pool, ctx, hidden, side):
        """side: (name, rows, dim) of the user-feature embeddings in front of the pooled vector (YouTubeRec)"""
        from ..modules import LatentFactor
        D, L = int(dim_item_embed), int(max_seq_len)
        if not 1 <= D <= 256:
            raise ValueError(f"{what}: dim_item_embed = {D} outside [1, 256]")
        if L < 1:
            raise ValueError(f"{what}: max_seq_len = {L}; at least 1")
        self.pool = ("fixed", L) if pool is None else pool
        rt._pool_arg(what, self.pool)
        self._set_l2_reg(0.0 if l2_reg_embed is None else l2_reg_embed)
        self.max_seq_len = L
        self.l2_reg_mlp = rt._coef_arg(what, "l2_reg_mlp", 0.0 if l2_reg_mlp is None else l2_reg_mlp)
        widths = None
        if hidden is not None or side:
            widths = [int(w) for w in hidden] if hidden is not None else []
            if not 1 <= len(widths) <= 4 or any(not 1 <= w <= 256 for w in widths):
                raise ValueError(f"{what}: hidden = {hidden!r}; 1 .. 4 widths, each in [1, 256]")
            widths = [sum(d for _, _, d in side) + D] + widths
            if widths[0] > 256:
                raise ValueError(f"{what}: the tower's input is {widths[0]} wide; at most 256")
        self.seq_item_latent_factor = LatentFactor(num_instances=total_items, dim=D, name='seq_item_latent_factor', ctx=ctx)
        ctx = self.seq_item_latent_factor.table.ctx
        Dq = widths[-1] if widths else D
        self.item_latent_factor = LatentFactor(num_instances=total_items, dim=Dq, name='item_latent_factor', ctx=ctx)
        self.item_bias = LatentFactor(num_instances=total_items, dim=1, name='item_bias', ctx=ctx) if use_item_bias else None
        self.user_latent_factor = None          # (the base class's name for the user side: this model pools it per call)
        self._queue = None
        self.user_features = [name for name, _, _ in side]
        self.user_feature_factors = [LatentFactor(num_instances=rows, dim=d, name='user_' + name, ctx=ctx) for name, rows, d in side]
        self.mlp_weights, self.mlp_biases = [], []
        tables = (self.seq_item_latent_factor.table, self.item_latent_factor.table, self.item_bias.table if self.item_bias is not None else None)
        if widths is None:
            self._net = rt.SeqRec(*tables, pool=self.pool)
        else:
            rng = np.random.default_rng(0)
            for l in range(len(widths) - 1):                 # Xavier-uniform weights, zero biases
                W = LatentFactor(num_instances=widths[l], dim=widths[l + 1], name=f'mlp_w{l}', ctx=ctx)
                a = np.sqrt(6.0 / (widths[l] + widths[l + 1]))
                W.table.write(rng.uniform(-a, a, (widths[l], widths[l + 1])).astype(np.float32))
                self.mlp_weights.append(W)
                self.mlp_biases.append(LatentFactor(num_instances=1, dim=widths[l + 1], zero_init=True, name=f'mlp_b{l}', ctx=ctx))
            self._net = rt.DeepSeqRec(*tables, [(W.table, c.table) for W, c in zip(self.mlp_weights, self.mlp_biases)],
                                      side=[lf.table for lf in self.user_feature_factors], pool=self.pool)
        self._deep = widths is not None
        self._history = None

    def _factors(self):
        return [lf for lf in (self.seq_item_latent_factor, self.item_latent_factor, self.item_bias, *self.user_feature_factors,
                              *self.mlp_weights, *self.mlp_biases) if lf is not None]

    def _side(self, user_features):
        """one id array per user feature, by the feature's name -> the lists in the tower's order"""
        if set(user_features) != set(self.user_features):
            raise ValueError(f"{type(self).__name__}: user features {sorted(user_features)} given; expected {sorted(self.user_features)}")
        return tuple(_ids(user_features[name]) for name in self.user_features)

    def _bags(self, seq_item_id, seq_len):
        seq, ln = _ids(seq_item_id), _ids(seq_len)
        shape = tuple(getattr(seq, "shape", ()))
        if len(shape) != 2 or shape[1] > self.max_seq_len:
            raise ValueError(f"{type(self).__name__}: seq_item_id shaped {shape}; expected [B, L] with L <= max_seq_len = {self.max_seq_len}")
        return (seq, ln)

    def train_steps(self, optimizer, seq_item_id, seq_len, label, n_item_id, loss="softmax", sample_weight=None, neg_offset=None,
                    want_loss=True, train=None):
        """One train step in one device call (rt.SeqRec.step): histories seq_item_id [B, L] of which seq_len [B] entries count,
        the next item label [B], negatives n_item_id [B, N].  loss: "softmax" | "logsig"; sample_weight [B]; neg_offset [B, N];
        train: None, or a subset of ("history", "item", "bias").  The objective is loss + l2_reg_embed * l2_loss.
        -> (loss[1], l2[1]) as float32 arrays when want_loss, else None"""
        if self._deep:
            raise NotImplementedError(f"{type(self).__name__}: with hidden layers the sampled-negatives step is not offered; use train_steps_full")
        opt = optimizer.native(self._net.ctx) if hasattr(optimizer, "native") else optimizer
        wts = _ids(sample_weight) if sample_weight is not None else None
        off = _ids(neg_offset) if neg_offset is not None else None
        return self._net.step(opt, self._bags(seq_item_id, seq_len), _ids(label), _ids(n_item_id), loss=loss, weights=wts,
                              neg_offset=off, l2_reg=self.l2_reg, train=train, want_loss=want_loss)

    def loss(self, seq_item_id, seq_len, label, n_item_id, loss="softmax", sample_weight=None, neg_offset=None):
        """the forward alone -> (loss, l2)"""
        if self._deep:
            raise NotImplementedError(f"{type(self).__name__}: with hidden layers the sampled-negatives loss is not offered; use loss_full")
        wts = _ids(sample_weight) if sample_weight is not None else None
        off = _ids(neg_offset) if neg_offset is not None else None
        return self._net.loss(self._bags(seq_item_id, seq_len), _ids(label), _ids(n_item_id), loss=loss, weights=wts, neg_offset=off)

    def train_steps_full(self, optimizer, seq_item_id, seq_len, label, sample_weight=None, item_offset=None, want_loss=True,
                         train=None, **user_features):
        """One train step on the reference's objective (rt.SeqRec.step_full): the softmax of the label over ALL items, no
        negatives to draw.  item_offset [total_items]: a per-item constant added to every row's logits (-inf removes an item,
        a padding id for one).  The item table and the bias take the optimizer's dense rule on every row.  With hidden layers
        (rt.DeepSeqRec.step_full) the layers take it too, `train` may also name "side" and "tower", and user_features holds one
        id array [B] per user feature, by name.
        -> (loss[1], l2[1]) as float32 arrays when want_loss, else None"""
        opt = optimizer.native(self._net.ctx) if hasattr(optimizer, "native") else optimizer
        wts = _ids(sample_weight) if sample_weight is not None else None
        off = _ids(item_offset) if item_offset is not None else None
        if self._deep:
            return self._net.step_full(opt, self._bags(seq_item_id, seq_len), _ids(label), self._side(user_features), weights=wts,
                                       item_offset=off, l2_reg=self.l2_reg, l2_mlp=self.l2_reg_mlp, train=train, want_loss=want_loss)
        self._side(user_features)
        return self._net.step_full(opt, self._bags(seq_item_id, seq_len), _ids(label), weights=wts, item_offset=off,
                                   l2_reg=self.l2_reg, train=train, want_loss=want_loss)

    def loss_full(self, seq_item_id, seq_len, label, sample_weight=None, item_offset=None, **user_features):
        """the forward of train_steps_full alone -> (loss, l2)"""
        wts = _ids(sample_weight) if sample_weight is not None else None
        off = _ids(item_offset) if item_offset is not None else None
        if self._deep:
            return self._net.loss_full(self._bags(seq_item_id, seq_len), _ids(label), self._side(user_features), weights=wts, item_offset=off)
        self._side(user_features)
        return self._net.loss_full(self._bags(seq_item_id, seq_len), _ids(label), weights=wts, item_offset=off)

    def _label_sets(self, label_item_id, label_len, label_weight):
        lab, ln = _ids(label_item_id), _ids(label_len)
        shape = tuple(getattr(lab, "shape", ()))
        if len(shape) != 2:
            raise ValueError(f"{type(self).__name__}: label_item_id shaped {shape}; expected the padded [B, L] beside label_len [B]")
        return (lab, ln), (_ids(label_weight) if label_weight is not None else None)

    def train_steps_sets(self, optimizer, seq_item_id, seq_len, label_item_id, label_len, label_weight=None, sample_weight=None,
                         item_offset=None, want_loss=True, train=None, **user_features):
        """train_steps_full with a label SET per history (rt.SeqRec.step_full(labels=...) / rt.DeepSeqRec.step_full(labels=...)):
        the multinomial likelihood of the history's whole set of items over ALL items, in one walk of the item table -- the
        objective of Mult-DAE.  label_item_id [B, Ll] of which label_len [B] entries count (an empty set keeps only its l2
        part); label_weight [B, Ll]: per-entry weights (None: 1).  Everything else as train_steps_full.
        -> (loss[1], l2[1]) as float32 arrays when want_loss, else None"""
        opt = optimizer.native(self._net.ctx) if hasattr(optimizer, "native") else optimizer
        wts = _ids(sample_weight) if sample_weight is not None else None
        off = _ids(item_offset) if item_offset is not None else None
        labels, lw = self._label_sets(label_item_id, label_len, label_weight)
        if self._deep:
            return self._net.step_full(opt, self._bags(seq_item_id, seq_len), None, self._side(user_features), weights=wts,
                                       item_offset=off, l2_reg=self.l2_reg, l2_mlp=self.l2_reg_mlp, train=train, want_loss=want_loss,
                                       labels=labels, label_weights=lw)
        self._side(user_features)
        return self._net.step_full(opt, self._bags(seq_item_id, seq_len), None, weights=wts, item_offset=off, l2_reg=self.l2_reg,
                                   train=train, want_loss=want_loss, labels=labels, label_weights=lw)

    def loss_sets(self, seq_item_id, seq_len, label_item_id, label_len, label_weight=None, sample_weight=None, item_offset=None,
                  **user_features):
        """the forward of train_steps_sets alone -> (loss, l2)"""
        wts = _ids(sample_weight) if sample_weight is not None else None
        off = _ids(item_offset) if item_offset is not None else None
        labels, lw = self._label_sets(label_item_id, label_len, label_weight)
        if self._deep:
            return self._net.loss_full(self._bags(seq_item_id, seq_len), None, self._side(user_features), weights=wts, item_offset=off,
                                       labels=labels, label_weights=lw)
        self._side(user_features)
        return self._net.loss_full(self._bags(seq_item_id, seq_len), None, weights=wts, item_offset=off, labels=labels, label_weights=lw)

    def _tables(self, flush=True):
        """what the scoring paths see: (the pooled rows of the histories last handed over, V, b)"""
        if self._history is None:
            raise ValueError(f"{type(self).__name__}: no histories to score (pass seq_item_id and seq_len)")
        if self._deep:
            return self._net.user_table(self._history, self._history_side), self._net.V, self._net.b
        return self._net.user_table(self._history), self._net.V, self._net.b

    def _rows(self, seq_item_id, seq_len, user_features=None):
        """the histories become the user table of the call that follows -> their row numbers, the ids that call takes"""
        self._history_side = self._side(user_features or {})
        self._history = self._bags(seq_item_id, seq_len)
        return np.arange(int(self._history[0].shape[0]), dtype=np.int32)

    def inference(self, seq_item_id, seq_len, **user_features):
        """q(history) @ V^T + b -> [B, total_items]"""
        uid = self._rows(seq_item_id, seq_len, user_features)
        Q, V, b = self._tables()
        return rt.score_all_items("dot", Q, V, b, uid, device=True)

    def recommend(self, seq_item_id, seq_len, k, excl_mask=None, **user_features):
        """the k best items of each history -> (item ids [B, k], scores [B, k]); see Recommender.recommend"""
        return super().recommend(self._rows(seq_item_id, seq_len, user_features), k, excl_mask)

    def score(self, seq_item_id, seq_len, candidates, **user_features):
        """the scores of each history's own candidate list; see Recommender.score"""
        return super().score(self._rows(seq_item_id, seq_len, user_features), candidates)

    def evaluate(self, seq_item_id, seq_len, pos_mask, excl_mask=None, at=(100,), score_matrix=True, cand_mask=None, **user_features):
        """AUC / NDCG / Recall of each history against its positives; see Recommender.evaluate"""
        return super().evaluate(self._rows(seq_item_id, seq_len, user_features), pos_mask, excl_mask, at, score_matrix, cand_mask)
