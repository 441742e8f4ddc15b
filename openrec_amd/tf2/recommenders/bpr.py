"""BPR (openrec/tf2/recommenders/bpr.py:5-43): same constructor, attributes,
call signature and return value `(loss, l2_loss)`; the five gathers, the
pairwise log loss, l2_loss and (under a tape) the gradients + optimizer update
run as one fused HIP kernel."""
from ._base import PairwiseRecommender, _ids
from ..modules import PairwiseLogLoss
from ... import runtime as rt


class BPR(PairwiseRecommender):
    _model = "bpr"

    def __init__(self, dim_user_embed, dim_item_embed, total_users, total_items, ctx=None, use_item_bias=True, l2_reg=1.0):
        """l2_reg: the call returns (loss, l2_reg * l2_loss), so a tape over the tuple trains loss + l2_reg * l2_loss; 1.0 is
        the reference.  use_item_bias=False: no item-bias table (`item_bias` is None) -- the reference's PairwiseLogLoss without its
        two bias arguments (pairwise_log_loss.py:26-30), score u.p - u.n; inference U[uid] @ V^T."""
        self._build_tables(dim_user_embed, dim_item_embed, total_users, total_items, ctx, item_bias=use_item_bias)
        self.pairwise_log_loss = PairwiseLogLoss()
        self._set_l2_reg(l2_reg)

    def inference(self, user_id):
        """bpr.py:39-43:  U[user_id] @ V^T + b  -> [B, total_items] (no "+ b" without item biases)."""
        U, V, b = self._tables()
        return rt.score_all_items("dot", U, V, b, _ids(user_id), device=True)
