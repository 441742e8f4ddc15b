"""The expected result of a train step over a subset of a model's tables, composed from the oracle's own pieces
(oracle/numpy_oracle.py): gradients on the pre-step tables, `opt.begin_step()` where the optimizer has one, then `opt.apply`
for the trained roles only.  Shared by the GPU tests and by the CPU test that holds this composition to the fixtures minted
from the reference's class text (tests/golden/make_golden_subset.py)."""
import numpy as np


class Momentum:
    """keras.optimizers.SGD(lr, momentum > 0, nesterov) of TF 2.0.1 in NumPy (the restatement tests/keras_momentum.py holds,
    copied): duplicates summed first, a = a*m - lr*G, plain w += a, nesterov w += a*m - lr*G; untouched rows keep (w, a)."""
    kind = "momentum"

    def __init__(self, lr=0.01, momentum=0.9, nesterov=False):
        self.lr, self.momentum, self.nesterov = lr, momentum, bool(nesterov)
        self.vel = {}

    def apply(self, var, idx, grad, key=None):
        from oracle.numpy_oracle import _dedup_sum
        if key not in self.vel:
            self.vel[key] = np.zeros_like(var)
        a = self.vel[key]
        uniq, G = _dedup_sum(idx, grad)
        dt = var.dtype.type
        m, lr = dt(self.momentum), dt(self.lr)
        an = a[uniq] * m - lr * G
        var[uniq] = var[uniq] + ((an * m - lr * G) if self.nesterov else an)
        a[uniq] = an


def expect_step(model, U, V, b, ids, oo, roles, margin=0.5, a=2.0, b_w=0.5, sigmoid=False):
    """one step of the oracle on the trained roles only; returns (loss, l2).  U, V, b are updated in place."""
    from oracle import numpy_oracle as orc
    if model == "wrmf":
        uid, iid, lab = ids
        loss, l2, _ = orc.wrmf_forward(U, V, b, uid, iid, lab, a, b_w, sigmoid)
        gr = orc.wrmf_grads(U, V, b, uid, iid, lab, a, b_w, sigmoid)
        item_ids, gi, gb = iid, gr["gi"], gr["gb"][:, None]
    else:
        uid, pid, nid = ids
        if model == "bpr":
            loss, l2, _ = orc.bpr_forward(U, V, b, uid, pid, nid)
            gr = orc.bpr_grads(U, V, b, uid, pid, nid)
        else:
            loss, l2, _ = orc.ucml_forward(U, V, b, uid, pid, nid, margin)
            gr = orc.ucml_grads(U, V, b, uid, pid, nid, margin)
        item_ids = np.concatenate([pid, nid])
        gi = np.concatenate([gr["gp"], gr["gn"]]); gb = np.concatenate([gr["gbp"], gr["gbn"]])[:, None]
    if hasattr(oo, "begin_step"):
        oo.begin_step()
    if "user" in roles:
        oo.apply(U, uid, gr["gu"], key="U")
    if "item" in roles:
        oo.apply(V, item_ids, gi, key="V")
    if "bias" in roles:
        oo.apply(b, item_ids, gb, key="b")
    return loss, l2
