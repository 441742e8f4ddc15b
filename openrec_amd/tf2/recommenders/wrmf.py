"""WRMF (openrec/tf2/recommenders/wrmf.py:5-40): prediction = u . i + b_i,
confidence-weighted squared error summed over the batch
(modules/pointwise_mse_loss.py:18-31)."""
from ._base import PointwiseRecommender, _ids
from ..modules import PointwiseMSELoss
from ... import runtime as rt


class WRMF(PointwiseRecommender):

    def __init__(self, dim_user_embed, dim_item_embed, total_users, total_items, a=1.0, b=1.0, ctx=None, l2_reg=1.0):
        """l2_reg: the call returns (loss, l2_reg * l2_loss); 1.0 is the reference"""
        self._build_tables(dim_user_embed, dim_item_embed, total_users, total_items, ctx)
        self.pointwise_mse_loss = PointwiseMSELoss(a=a, b=b)
        self._a, self._b = a, b
        self._set_l2_reg(l2_reg)

    def _point_args(self):
        return "wrmf", None, dict(a=self._a, b_w=self._b)

    def fit_als(self, data, sweeps=1, reg=0.1, confidence=None, solver="cholesky", cg_steps=3):
        """Beyond the reference API: train by alternating least squares (Hu / Koren / Volinsky) instead of sampled SGD --
        `sweeps` times the user half-step then the item half-step of rt.als_sweep, each row solved in closed form over ALL
        cells with the model's own a (observed) and b (unobserved) as confidences.  `data`: the structured array the
        reference's Dataset takes, or an rt.ALSData built once; `confidence`: one float per record instead of `a` (only with
        raw data).  ALS here has no bias term while `inference` adds the item bias, so the bias table must be all zero:
        anything else is a ValueError.  solver="cg": every row takes `cg_steps` conjugate-gradient steps from its current value
        instead of the closed form (rt.als_half_step).  Returns self."""
        U, V, b = self._tables()
        sweeps = int(sweeps)
        if sweeps < 0:
            raise ValueError(f"fit_als: sweeps = {sweeps}")
        cg_steps = rt._als_solver("fit_als", solver, cg_steps)
        if isinstance(data, rt.ALSData):
            if confidence is not None:
                raise ValueError("fit_als: an ALSData carries its own confidences")
        else:
            data = rt.ALSData(data, U.rows, V.rows, confidence=confidence, ctx=U.ctx)
        if b.read().any():
            raise ValueError("fit_als: ALS has no bias term, but the item-bias table is not all zero (fill it with 0 first)")
        for _ in range(sweeps):
            rt.als_sweep(U, V, data, self._a, self._b, reg, solver=solver, cg_steps=cg_steps)
        return self

    def als_objective(self, data, reg=0.1):
        """What fit_als descends, computed on the device (rt.als_objective) with the model's a and b: `data` an rt.ALSData or
        the structured array it is built from.  -> float"""
        U, V, _ = self._tables()
        if not isinstance(data, rt.ALSData):
            data = rt.ALSData(data, U.rows, V.rows, ctx=U.ctx)
        return rt.als_objective(U, V, data, self._a, self._b, reg)

    def inference(self, user_id):
        """wrmf.py:36-40:  U[user_id] @ V^T + b."""
        U, V, b = self._tables()
        return rt.score_all_items("dot", U, V, b, _ids(user_id), device=True)
