"""LightGCN (He et al., SIGIR 2020), beyond the reference's model list: BPR whose scored rows are the embeddings propagated over
the user-item graph, E_f = sum_k alpha_k A~^k [U ; V] (rt.LightGCN).  The two trainable tables are LatentFactors as in the other
recommenders; there is no item bias.  Training goes through `train_steps` (no tape); `inference`, `recommend`, `score` and
`evaluate` run on the PROPAGATED tables through the paths the other recommenders use.  The propagation is redone when
`train_steps` has run since the last one; a change of the two tables from anywhere else (writing a LatentFactor's table, loading
a checkpoint, rt.pairwise_step on the tables) is NOT noticed: call `invalidate()` after it."""
import numpy as np

from ._base import Recommender, _ids
from ... import runtime as rt


class LightGCN(Recommender):

    def __init__(self, dim, total_users, total_items, layers=3, l2_reg=1e-4, ctx=None, layer_weights=None):
        """layers: propagation depth L in [1, 8]; layer_weights: L + 1 floats, 1 / (L + 1) each by default; l2_reg: the
        coefficient of the l2 term of the batch's layer-0 rows (the paper's form, divided by the batch size)"""
        layers = int(layers)
        if not 1 <= layers <= rt.LIGHTGCN_MAX_LAYERS:
            raise ValueError(f"LightGCN: layers = {layers} outside [1, {rt.LIGHTGCN_MAX_LAYERS}]")
        if layer_weights is not None and len(layer_weights) != layers + 1:
            raise ValueError(f"LightGCN: {len(layer_weights)} layer weights for {layers} layers")
        if not 1 <= int(dim) <= 128:
            raise ValueError(f"LightGCN: dim {dim} outside [1, 128]")
        self._build_tables(dim, dim, total_users, total_items, ctx, item_bias=False)
        self.layers, self.layer_weights = layers, layer_weights
        self._set_l2_reg(l2_reg)
        self.graph = self._net = None

    def fit_graph(self, data):
        """the interaction set the model propagates over: the structured array ('user_id', 'item_id') the reference's Dataset
        takes, an rt.ALSData or an rt.InteractionGraph.  Returns self."""
        U, V, _ = Recommender._tables(self)
        if not isinstance(data, rt.InteractionGraph):
            data = rt.InteractionGraph(data, None if isinstance(data, rt.ALSData) else U.rows,
                                       None if isinstance(data, rt.ALSData) else V.rows, ctx=U.ctx)
        self._net = rt.LightGCN(U, V, data, layers=self.layers, layer_weights=self.layer_weights)
        self.graph = data
        return self

    def _need_graph(self, what):
        if self._net is None:
            raise RuntimeError(f"LightGCN.{what}: no graph yet (call fit_graph first)")
        return self._net

    def invalidate(self):
        """the tables were changed by anything but `train_steps`: the next scoring call propagates again (nothing else tells
        the model, it would go on serving the tables of its last propagation)"""
        if self._net is not None:
            self._net.invalidate()

    def _tables(self, flush=True):
        """what the scoring paths see: the propagated tables, brought up to date when a step has run since"""
        Uf, Vf = self._need_graph("scoring").propagate()
        return Uf, Vf, None

    def propagated(self):
        """-> (Uf, Vf) as rt.Tables (valid until the next step)"""
        return self._tables()[:2]

    def train_steps(self, optimizer, user_id, p_item_id, n_item_id, K=None, want_loss=True, train=None):
        """K consecutive train steps (ids shaped [K, B], or [B]: one step), each rt.LightGCN.step with the model's l2_reg.
        -> (loss[K], l2[K]) as float32 arrays when want_loss, else None"""
        net = self._need_graph("train_steps")
        uid, pid, nid = _ids(user_id), _ids(p_item_id), _ids(n_item_id)
        if K is None:
            K = uid.shape[0] if getattr(uid, "ndim", 1) == 2 else 1
        if getattr(uid, "ndim", 1) != 2:
            uid, pid, nid = (x.reshape(K, -1) for x in (uid, pid, nid))
        opt = optimizer.native(net.ctx) if hasattr(optimizer, "native") else optimizer
        loss, l2 = np.zeros(K, np.float32), np.zeros(K, np.float32)
        for k in range(K):
            out = net.step(opt, uid[k], pid[k], nid[k], l2_reg=self.l2_reg, train=train, want_loss=want_loss)
            if want_loss:
                loss[k], l2[k] = out
        return (loss, l2) if want_loss else None

    def loss(self, user_id, p_item_id, n_item_id):
        """the forward alone -> (loss, l2)"""
        return self._need_graph("loss").loss(_ids(user_id), _ids(p_item_id), _ids(n_item_id), l2_reg=self.l2_reg)

    def inference(self, user_id):
        """Uf[user_id] @ Vf^T -> [B, total_items]"""
        Uf, Vf, _ = self._tables()
        return rt.score_all_items("dot", Uf, Vf, None, _ids(user_id), device=True)
