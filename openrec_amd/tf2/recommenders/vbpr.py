"""VBPR (He & McAuley, AAAI 2016; the reference's tf1/recommenders/vbpr.py): BPR whose item vector is the latent row beside a learned
projection of a fixed per-item feature vector (rt.VBPR),
    s(u, i) = U[u, :Dl] . V[i] + U[u, Dl:] . (F[i] E) + b[i].
The projection is one linear layer WITHOUT an output bias: the reference's Dense layer has one, but it cancels in every pair
difference, its loss gradient is identically zero, and in serving it shifts all items of a user equally.  The tables are
LatentFactors as in the other recommenders, the projection E [Fd, Dc] among them.  Training goes through `train_steps` (no tape);
`inference`, `recommend`, `score` and `evaluate` run on (U, [V | F E], b) through the paths the other recommenders use.  The item
table is rebuilt when `train_steps` has run since the last build; a change of V, E or the features from anywhere else (writing a
LatentFactor's table, loading a checkpoint) is NOT noticed: call `invalidate()` after it (`set_item_features` does)."""
import numpy as np

from ._base import Recommender, _StepQueue, _ids
from ... import runtime as rt


class VBPR(Recommender):

    def __init__(self, dim_user_embed, dim_item_embed, total_users, total_items, item_features, l2_reg=None, l2_reg_mlp=None,
                 use_item_bias=True, ctx=None):
        """dim_item_embed: the latent width Dl; the projection width is Dc = dim_user_embed - dim_item_embed, as in the
        reference's signature.  item_features: float32 [total_items, Fd] (NumPy, a torch device tensor, or an rt.ItemFeatures).
        l2_reg: the coefficient of the l2 term of the looked-up rows (None: 0); l2_reg_mlp: of 1/2 |E|^2 (None: 0)."""
        from ..modules import LatentFactor
        what = "VBPR"
        Dl, D = int(dim_item_embed), int(dim_user_embed)
        Dc = D - Dl
        if Dl < 1:
            raise ValueError(f"{what}: dim_item_embed = {Dl}; the latent width must be at least 1")
        if not 1 <= Dc <= 128:
            raise ValueError(f"{what}: the projection width dim_user_embed - dim_item_embed = {Dc} must be in [1, 128]")
        if D > 256:
            raise ValueError(f"{what}: dim_user_embed = {D} above 256")
        rows = item_features.rows if isinstance(item_features, rt.ItemFeatures) else int(np.shape(item_features)[0])
        if rows != int(total_items):
            raise ValueError(f"{what}: {rows} feature rows for {int(total_items)} items")
        l2p = float(0.0 if l2_reg_mlp is None else l2_reg_mlp)
        if not (np.isfinite(l2p) and l2p >= 0):
            raise ValueError(f"{what}: l2_reg_mlp must be finite and >= 0, got {l2_reg_mlp!r}")
        self._set_l2_reg(0.0 if l2_reg is None else l2_reg)
        feats = item_features if isinstance(item_features, rt.ItemFeatures) else rt.ItemFeatures(item_features, ctx)
        ctx = feats.ctx
        self.user_latent_factor = LatentFactor(num_instances=total_users, dim=D, name='user_latent_factor', ctx=ctx)
        self.item_latent_factor = LatentFactor(num_instances=total_items, dim=Dl, name='item_latent_factor', ctx=ctx)
        self.item_bias = LatentFactor(num_instances=total_items, dim=1, name='item_bias', ctx=ctx) if use_item_bias else None
        self.projection = LatentFactor(num_instances=feats.dim, dim=Dc, name='projection', ctx=ctx)
        self._queue = _StepQueue()
        self.item_features = feats
        self.l2_reg_mlp = l2p
        self._net = rt.VBPR(self.user_latent_factor.table, self.item_latent_factor.table,
                            self.item_bias.table if self.item_bias is not None else None, self.projection.table, feats)

    def _factors(self):
        return [lf for lf in (self.user_latent_factor, self.item_latent_factor, self.item_bias, self.projection) if lf is not None]

    def invalidate(self):
        """V, E or the features were changed by anything but `train_steps` / `set_item_features`: the next scoring call rebuilds
        the item table (nothing else tells the model, it would go on serving its last one)"""
        self._net.invalidate()

    def set_item_features(self, rows, values):
        """F[rows] = values: the feature rows of newly arrived items; their vectors [V | F E] are in place at the next scoring call"""
        self.item_features.write_rows(rows, values)
        self._net.invalidate()

    def _tables(self, flush=True):
        """what the scoring paths see: (U, [V | F E], b), the item table brought up to date when a step has run since"""
        return self._net.U, self._net.item_table(), self._net.b

    def train_steps(self, optimizer, user_id, p_item_id, n_item_id, sample_weight=None, K=None, want_loss=True, train=None):
        """K consecutive train steps in one device call (ids shaped [K, B], or [B]: one step): rt.VBPR.step with the model's
        l2_reg and l2_reg_mlp.  train: None, or a subset of ("user", "item", "bias", "proj").
        -> (loss[K], l2[K]) as float32 arrays when want_loss, else None"""
        uid, pid, nid = _ids(user_id), _ids(p_item_id), _ids(n_item_id)
        if K is None:
            K = uid.shape[0] if getattr(uid, "ndim", 1) == 2 else 1
        opt = optimizer.native(self._net.ctx) if hasattr(optimizer, "native") else optimizer
        wts = _ids(sample_weight) if sample_weight is not None else None
        return self._net.step(opt, uid, pid, nid, weights=wts, l2_reg=self.l2_reg, l2_proj=self.l2_reg_mlp, train=train, K=K,
                              want_loss=want_loss)

    def loss(self, user_id, p_item_id, n_item_id, sample_weight=None):
        """the forward alone -> (loss, l2)"""
        wts = _ids(sample_weight) if sample_weight is not None else None
        return self._net.loss(_ids(user_id), _ids(p_item_id), _ids(n_item_id), weights=wts)

    def inference(self, user_id):
        """U[user_id] @ [V | F E]^T + b -> [B, total_items]"""
        U, W, b = self._tables()
        return rt.score_all_items("dot", U, W, b, _ids(user_id), device=True)
