"""keras.optimizers.SGD(lr, momentum > 0, nesterov) of TF 2.0.1, restated in NumPy for the tests.

Sparse variables: _resource_apply_sparse_duplicate_indices sums the duplicates first, then ResourceSparseApplyKerasMomentum
updates each unique row i with summed gradient G and velocity a:
    a[i] = a[i]*momentum - lr*G;   plain: w[i] += a[i];   nesterov: w[i] += a[i]*momentum - lr*G
Rows not referenced are untouched, velocity included.  Dense variables (ResourceApplyKerasMomentum): the same rule on
every element.  The "momentum" slot is zero-initialised.  Every product and sum rounds in the variable's dtype, as TF's
kernels do.

Duck-typed like oracle/numpy_oracle.py's optimizers (`kind`, `apply`, `apply_dense`), so the oracle's train steps
(bpr_step / ucml_step / gmf_step / wrmf_step, DLRMOracle.step) drive it unchanged."""
import numpy as np

from oracle.numpy_oracle import _dedup_sum


class Momentum:
    kind = "momentum"

    def __init__(self, lr=0.01, momentum=0.9, nesterov=False):
        if not 0.0 <= momentum <= 1.0:
            raise ValueError("`momentum` must be between [0, 1].")
        self.lr, self.momentum, self.nesterov = lr, momentum, bool(nesterov)
        self.vel = {}

    def slot(self, var, key=None):
        key = id(var) if key is None else key
        if key not in self.vel:
            self.vel[key] = np.zeros_like(var)
        return self.vel[key]

    def _rule(self, w, a, G):
        """(new w, new a) of the rows / elements w with velocity a and summed gradient G"""
        dt = w.dtype.type
        m, lr = dt(self.momentum), dt(self.lr)
        a = a * m - lr * G
        if self.nesterov:
            return w + (a * m - lr * G), a
        return w + a, a

    def apply(self, var, idx, grad, key=None):
        a = self.slot(var, key)
        uniq, G = _dedup_sum(idx, grad)
        var[uniq], a[uniq] = self._rule(var[uniq], a[uniq], G)

    def apply_dense(self, var, grad, key=None):
        a = self.slot(var, key)
        w, an = self._rule(var, a, grad.astype(var.dtype))
        var[...] = w
        a[...] = an
