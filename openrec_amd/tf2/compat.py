"""The handful of TensorFlow symbols that `tf2_examples/*.py` touch around the
hot path, so that a script shaped like
tf2_examples/bpr_citeulike.py runs with only its imports changed:

    from openrec_amd.tf2.compat import tf, optimizers
    from openrec_amd.tf2.recommenders import BPR

`install()` additionally registers this module as `tensorflow` in sys.modules --
only when no real TensorFlow is importable; it never shadows one."""
from __future__ import annotations

import collections
import sys
import types
import weakref

import numpy as np

from .. import runtime as rt
from ._lazy import GradientTape, GradToken, LazyScalar


def function(fn=None, **_):
    """tf.function: the fused step is already one device call, nothing to trace."""
    if fn is None:
        return lambda f: f
    return fn


def constant(value, dtype=None):
    return np.asarray(value, dtype=dtype)


int32, float32, bool_ = np.int32, np.float32, np.bool_


class _Optimizer:
    """Keras optimizer facade; the device-side state lives in runtime.Optimizer."""
    _kind = None

    def __init__(self):
        self._native = None
        self._models = weakref.WeakSet()       # models with steps applied through this optimizer (their queues hold it)
        self._lr = None
        self._iterations = 0

    def _make(self, ctx):
        raise NotImplementedError

    def native(self, ctx=None):
        if self._native is None:
            self._native = self._make(ctx)
        return self._native

    def _flush_models(self):
        for m in list(self._models):
            flush = getattr(m, "flush", None)
            if flush is not None:
                flush()

    # Keras `optimizer.learning_rate` (also `.lr`): assignable at any time.  Steps already applied -- queued or not --
    # keep the rate they were applied with: the queues run first, then the device-side optimizer takes the new rate.
    @property
    def learning_rate(self):
        return self._lr

    @learning_rate.setter
    def learning_rate(self, value):
        value = float(value)
        if self._native is not None and value != self._lr:
            self._flush_models()
            self._native.set_lr(value)
        self._lr = value

    lr = learning_rate

    @property
    def iterations(self):
        """Keras `optimizer.iterations`: steps applied so far (the queued ones included).  An Adam optimizer keeps the
        counter natively (it is part of a checkpoint, runtime.load_checkpoint restores it): the queues run, then the
        native counter answers."""
        if self._native is not None and self._native.kind == "adam":
            self._flush_models()
            return self._native.step
        return self._iterations

    def apply_gradients(self, grads_and_vars):
        """Consumes the tokens of `GradientTape.gradient`: all tokens of one recorded
        step trigger ONE fused forward+backward+update call.  As in Keras, only the variables handed over are updated:
        a strict subset of the step's model (`layer.trainable = False`, a shorter variable list) trains those tables and
        leaves the others, and their optimizer slots, untouched."""
        steps = []                              # [step, no_l2, variables]
        for g, v in grads_and_vars:
            if not isinstance(g, GradToken):
                raise TypeError("apply_gradients expects gradients produced by openrec_amd's GradientTape")
            for entry in steps:
                if entry[0] is g.step:
                    entry[2].append(v)
                    break
            else:
                steps.append([g.step, g.no_l2, [v]])
        plans = [(step, no_l2, _train_subset(step.model, variables)) for step, no_l2, variables in steps]      # (raises before any step runs)
        for step, no_l2, train in plans:
            ctx = step.model.user_latent_factor.table.ctx
            self._models.add(step.model)
            step.train(self.native(ctx), no_l2, train)
            self._iterations += 1


def _train_subset(model, variables):
    """The variables handed to apply_gradients for a step of `model` -> None (all of the model's: the full step) or the roles
    of a strict subset ("user" / "item" / "bias").  Every model maps variables to its parameters by TABLE identity
    (`_train_roles`); a variable that is not the model's is a ValueError, a strict subset a model cannot train raises
    NotImplementedError."""
    return model._train_roles(variables)


class SGD(_Optimizer):
    """keras.optimizers.SGD(learning_rate, momentum, nesterov).  momentum == 0: plain SGD (every occurrence accumulated);
    momentum > 0: the momentum rule of TF 2.0 (duplicates summed first, one "momentum" slot per variable)."""

    def __init__(self, learning_rate=0.01, momentum=0.0, nesterov=False, **_):
        super().__init__()
        momentum = float(momentum)
        if not 0.0 <= momentum <= 1.0:                  # (as keras raises it; a NaN is refused too)
            raise ValueError("`momentum` must be between [0, 1].")
        self.momentum, self.nesterov = momentum, bool(nesterov)
        self.learning_rate = learning_rate

    def _make(self, ctx):
        if self.momentum > 0:
            return rt.Optimizer.momentum(self.learning_rate, self.momentum, self.nesterov, ctx=ctx)
        return rt.Optimizer.sgd(self.learning_rate, ctx=ctx)


class Adagrad(_Optimizer):
    def __init__(self, learning_rate=0.001, initial_accumulator_value=0.1, epsilon=1e-7, **_):
        super().__init__()
        self.learning_rate, self.iav, self.epsilon = learning_rate, initial_accumulator_value, epsilon

    def _make(self, ctx):
        return rt.Optimizer.adagrad(self.learning_rate, self.iav, self.epsilon, ctx=ctx)


class Adam(_Optimizer):
    """keras.optimizers.Adam() as used by tf2_examples/bpr_citeulike.py:31 (TF-2.0
    dense-decay sparse apply)."""

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, **_):
        super().__init__()
        self.learning_rate, self.beta_1, self.beta_2, self.epsilon = learning_rate, beta_1, beta_2, epsilon

    def _make(self, ctx):
        return rt.Optimizer.adam(self.learning_rate, self.beta_1, self.beta_2, self.epsilon, ctx=ctx)


class HostTensor(np.ndarray):
    """What the metric objects hand back: an ndarray that also answers `.numpy()`, as the reference scripts print
    `average_loss.result().numpy()` / `result['AUC'].numpy()` (tf2_examples/bpr_citeulike.py:64-65)."""

    def __new__(cls, value, dtype=np.float32):
        return np.asarray(value, dtype=dtype).view(cls)

    def numpy(self):
        return np.asarray(self)


class Mean:
    """tf.keras.metrics.Mean; `update_state((loss, l2))` averages the two scalars
    together, like the reference script does (bpr_citeulike.py:54)."""

    def __init__(self):
        self.reset_states()

    def update_state(self, values):
        for v in (values if isinstance(values, (tuple, list)) else [values]):
            if isinstance(v, LazyScalar):
                self._pending.append(v)         # reading it now would force the queued train steps to run
                if len(self._pending) > 4096:
                    self._drain()
                continue
            a = np.asarray(v.numpy() if hasattr(v, "numpy") else v, np.float64)
            self._sum += float(a.sum())
            self._n += a.size

    __call__ = update_state

    def _drain(self):
        for v in self._pending:
            self._sum += float(v.numpy())
            self._n += 1
        self._pending = []

    def result(self):
        self._drain()
        return HostTensor(self._sum / max(self._n, 1))

    def reset_states(self):
        self._sum, self._n, self._pending = 0.0, 0, []


class AUC:
    """tf.keras.metrics.AUC() with its defaults (200 thresholds, ROC, 'interpolation' = trapezoids), the validation metric of
    tf2_examples/dlrm_criteo.py:40, :50-53, :67.  Evaluation side of the script, host arithmetic."""

    def __init__(self, num_thresholds=200):
        n = int(num_thresholds)
        eps = 1e-7                                                   # keras: first / last threshold just outside [0, 1]
        self._thr = np.array([0.0 - eps] + [(i + 1) / (n - 1) for i in range(n - 2)] + [1.0 + eps])
        self.reset_states()

    def reset_states(self):
        self._tp = np.zeros(len(self._thr)); self._fp = np.zeros(len(self._thr))
        self._tn = np.zeros(len(self._thr)); self._fn = np.zeros(len(self._thr))

    def update_state(self, y_true, y_pred, sample_weight=None):
        y = np.asarray(y_true.numpy() if hasattr(y_true, "numpy") else y_true).reshape(-1) > 0
        p = np.asarray(y_pred.numpy() if hasattr(y_pred, "numpy") else y_pred, np.float64).reshape(-1)
        ps, ns = np.sort(p[y]), np.sort(p[~y])
        above_p = len(ps) - np.searchsorted(ps, self._thr, side="right")       # predictions > threshold
        above_n = len(ns) - np.searchsorted(ns, self._thr, side="right")
        self._tp += above_p; self._fn += len(ps) - above_p
        self._fp += above_n; self._tn += len(ns) - above_n

    def result(self):
        tpr = self._tp / np.maximum(self._tp + self._fn, 1e-7)
        fpr = self._fp / np.maximum(self._fp + self._tn, 1e-7)
        return HostTensor(np.sum((fpr[:-1] - fpr[1:]) * (tpr[:-1] + tpr[1:]) / 2.0))


class TensorSliceDataset:
    """tensorflow.data.Dataset as tf2_examples/dlrm_criteo.py:18-29 uses it: from_tensor_slices(dict) .batch .prefetch
    .shuffle, iterated once per epoch.  `shuffle(k)` after `batch` shuffles BATCHES through a k-element buffer, reshuffled
    at every iteration (TF's reshuffle_each_iteration default)."""

    def __init__(self, arrays, batch=None, shuffle=None, seed=None):
        self._arrays, self._batch, self._shuffle = arrays, batch, shuffle
        self._rng = np.random.default_rng(seed)

    @classmethod
    def from_tensor_slices(cls, tensors):
        arrays = {k: np.asarray(v.numpy() if hasattr(v, "numpy") else v) for k, v in dict(tensors).items()}
        n = {len(v) for v in arrays.values()}
        if len(n) != 1:
            raise ValueError("from_tensor_slices: components differ in their first dimension")
        return cls(arrays)

    def batch(self, batch_size, drop_remainder=False):
        d = TensorSliceDataset(self._arrays, int(batch_size), self._shuffle)
        d._drop = drop_remainder
        return d

    def prefetch(self, _buffer_size):
        return self

    def shuffle(self, buffer_size, seed=None, reshuffle_each_iteration=True):
        d = TensorSliceDataset(self._arrays, self._batch, int(buffer_size), seed)
        d._drop = getattr(self, "_drop", False)
        return d

    def _elements(self):
        n = len(next(iter(self._arrays.values())))
        if self._batch is None:
            for i in range(n):
                yield {k: v[i] for k, v in self._arrays.items()}
            return
        for lo in range(0, n, self._batch):
            if lo + self._batch > n and getattr(self, "_drop", False):
                return
            yield {k: v[lo:lo + self._batch] for k, v in self._arrays.items()}

    def __iter__(self):
        if not self._shuffle:
            yield from self._elements()
            return
        buf = []
        for e in self._elements():                      # TF's shuffle: fill the buffer, then emit a random slot per new element
            if len(buf) < self._shuffle:
                buf.append(e)
                continue
            j = int(self._rng.integers(len(buf)))
            out, buf[j] = buf[j], e
            yield out
        while buf:
            yield buf.pop(int(self._rng.integers(len(buf))))


class Model:
    """tensorflow.keras.Model as the reference's recommender classes use it (recommenders/bpr.py:5-9: subclass, assign
    modules as attributes, define `call`): `model(...)` runs `call`, `trainable_variables` collects the variables of the
    attributes in assignment order."""

    def __init__(self, *_, **__):
        pass

    def __call__(self, *args, **kwargs):
        kwargs.pop("training", None)
        return self.call(*args, **kwargs)

    def _collect(self, attr):
        out, seen = [], set()
        for v in vars(self).values():
            # (Keras tracks lists of layers too: dlrm.py:30-31 keeps its latent factors in one)
            for mod in (v if isinstance(v, (list, tuple)) else [v]):
                found = getattr(mod, attr, None)
                if found is None:                   # (a module that only knows one of the two names)
                    found = getattr(mod, "variables" if attr == "trainable_variables" else "trainable_variables", None) or []
                for var in found:
                    if id(var) not in seen:
                        seen.add(id(var))
                        out.append(var)
        return out

    @property
    def trainable_variables(self):
        """the variables of the attributes whose `trainable` is set (a LatentFactor with `trainable = False` has none)"""
        return self._collect("trainable_variables")

    @property
    def variables(self):
        return self._collect("variables")


class _AllItemScores:
    """`tf.linalg.matmul(user_vec, V, transpose_b=True)` of looked-up user rows and a whole item table (bpr.py:42):
    stays symbolic until the bias row is added, then runs the all-item scorer on the device."""

    def __init__(self, rows, item_var):
        self.rows, self.item_var = rows, item_var

    def __add__(self, other):
        from .modules.latent_factor import Variable
        bias = getattr(other, "flat_of", None)
        if isinstance(bias, Variable) and bias.table.dim == 1 and bias.table.rows == self.item_var.table.rows:
            ids = self.rows.flat_ids()
            self.rows.consumed()         # (scored in HBM: the lookup is never gathered to the host)
            return rt.score_all_items("dot", self.rows.factor.table, self.item_var.table, bias.table, ids, device=True)
        return HostTensor(np.asarray(self) + np.asarray(other))

    __radd__ = __add__

    def __array__(self, dtype=None, copy=None):
        a = np.asarray(self.rows, np.float32) @ self.item_var.numpy().T
        return a.astype(dtype) if dtype is not None else a

    def numpy(self):
        return np.asarray(self)


class _Flat:
    """tf.reshape(variable, [-1]): symbolic (the table stays in HBM) until something needs the values"""

    def __init__(self, var, shape):
        self.var, self.shape_arg = var, shape
        self.flat_of = var if list(np.atleast_1d(shape)) == [-1] else None

    def __array__(self, dtype=None, copy=None):
        a = self.var.numpy().reshape(self.shape_arg)
        return a.astype(dtype) if dtype is not None else a

    def numpy(self):
        return np.asarray(self)

    def __add__(self, other):
        if isinstance(other, _AllItemScores):
            return other.__add__(self)
        return np.asarray(self) + np.asarray(other)

    __radd__ = __add__


def matmul(a, b, transpose_a=False, transpose_b=False):
    from .modules.latent_factor import GatheredRows, Variable
    if isinstance(a, GatheredRows) and isinstance(b, Variable) and transpose_b and not transpose_a and a.ndim == 2 \
            and a.factor.dim == b.table.dim:
        return _AllItemScores(a, b)
    a = np.asarray(a.numpy() if isinstance(a, Variable) else a, np.float32)
    b = np.asarray(b.numpy() if isinstance(b, Variable) else b, np.float32)
    return HostTensor((a.T if transpose_a else a) @ (b.T if transpose_b else b))


def reshape(x, shape):
    from .modules.latent_factor import Variable
    from .modules._expr import Expr
    if isinstance(x, Variable):
        return _Flat(x, shape)
    if isinstance(x, Expr):
        return Expr("reshape", x, shape=shape)
    return np.asarray(x).reshape(shape)


def _expr_ops():
    from .modules import _expr
    return _expr


def _square(x): return _expr_ops().square(x)
def _reduce_sum(x, axis=None, keepdims=False): return _expr_ops().reduce_sum(x, axis=axis, keepdims=keepdims)
def _maximum(a, b): return _expr_ops().maximum(a, b)
def _expand_dims(x, axis): return _expr_ops().expand_dims(x, axis)
def _squeeze(x, axis=None): return _expr_ops().squeeze(x, axis=axis)


def _concat(values, axis): return _expr_ops().concat(values, axis)
def _clip_by_value(x, clip_value_min, clip_value_max): return _expr_ops().clip_by_value(x, clip_value_min, clip_value_max)
def _unstack(value, num=None, axis=0): return _expr_ops().unstack(value, axis=axis)


class _BCE:
    def __new__(cls, *a, **k):
        return _expr_ops().BinaryCrossentropy(*a, **k)


class _MSE:
    def __new__(cls, *a, **k):
        return _expr_ops().MeanSquaredError()


def _l2_loss(x):
    from .modules._compose import l2_loss
    return l2_loss(x)


TopKV2 = collections.namedtuple("TopKV2", ["values", "indices"])


def top_k(input, k=1, sorted=True, name=None):
    """tf.math.top_k over the last axis of a 1-D or 2-D input (a DeviceScores is read in HBM): the k largest values per
    row, ties to the lower index.  NaN entries are never returned (a row with fewer than k others ends in index -1 /
    -inf), and k is at most 1024.  The result is always sorted."""
    shape = tuple(input.shape) if hasattr(input, "shape") else np.shape(input)
    if len(shape) not in (1, 2):
        raise NotImplementedError(f"top_k: input of rank {len(shape)}; only rank 1 and 2 are supported")
    k = int(k)
    if k < 0:
        raise ValueError(f"top_k: k = {k} must be non-negative")
    if k > shape[-1]:
        raise ValueError(f"top_k: input must have at least k = {k} columns, has {shape[-1]}")
    if k == 0:
        rows = shape[:-1] + (0,)
        return TopKV2(HostTensor(np.zeros(rows), np.float32), HostTensor(np.zeros(rows), np.int32))
    rows = input if len(shape) == 2 else (input.reshape(1, -1) if _is_torch(input) else np.asarray(input).reshape(1, -1))
    idx, val = rt.topk_rows(rows, k)
    if len(shape) == 1:
        idx, val = idx[0], val[0]
    return TopKV2(HostTensor(val, np.float32), HostTensor(idx, np.int32))


def _is_torch(x):
    return hasattr(x, "data_ptr") and hasattr(x, "reshape") and getattr(x, "is_cuda", False)


optimizers = types.SimpleNamespace(SGD=SGD, Adagrad=Adagrad, Adam=Adam)
losses = types.SimpleNamespace(BinaryCrossentropy=_BCE, MeanSquaredError=_MSE)
keras = types.SimpleNamespace(optimizers=optimizers, metrics=types.SimpleNamespace(Mean=Mean, AUC=AUC), Model=Model, losses=losses)
math = types.SimpleNamespace(square=_square, reduce_sum=_reduce_sum, maximum=_maximum, top_k=top_k)
data = types.SimpleNamespace(Dataset=TensorSliceDataset)
nn = types.SimpleNamespace(l2_loss=_l2_loss, top_k=top_k)
linalg = types.SimpleNamespace(matmul=matmul)
tf = types.SimpleNamespace(function=function, GradientTape=GradientTape, constant=constant, keras=keras, data=data, nn=nn,
                           linalg=linalg, matmul=matmul, reshape=reshape, int32=int32, float32=float32, bool=bool_,
                           math=math, reduce_sum=_reduce_sum, maximum=_maximum, square=_square, expand_dims=_expand_dims, squeeze=_squeeze,
                           concat=_concat, clip_by_value=_clip_by_value, unstack=_unstack)


def install():
    """Make `import tensorflow as tf` / `from tensorflow.keras import optimizers` / `from tensorflow.data import Dataset`
    resolve to this shim when (and only when) TensorFlow is absent, and `openrec.tf2.{data, recommenders, metrics, modules}`
    to this package when the reference package is absent -- what an unmodified tf2_examples script imports
    (tf2_examples/bpr_citeulike.py:1-7, dlrm_criteo.py:1-5).  Returns True if the TensorFlow shim was installed."""
    install_openrec_alias()
    try:
        import tensorflow  # noqa: F401
        return False
    except Exception:
        pass
    mod = types.ModuleType("tensorflow")
    for k, v in vars(tf).items():
        setattr(mod, k, v)
    kmod = types.ModuleType("tensorflow.keras")
    kmod.optimizers, kmod.metrics, kmod.Model, kmod.losses = optimizers, keras.metrics, Model, losses
    omod = types.ModuleType("tensorflow.keras.optimizers")
    omod.SGD, omod.Adagrad, omod.Adam = SGD, Adagrad, Adam
    mmod = types.ModuleType("tensorflow.keras.metrics")
    mmod.Mean, mmod.AUC = Mean, AUC
    dmod = types.ModuleType("tensorflow.data")
    dmod.Dataset = TensorSliceDataset
    mod.keras, mod.data = kmod, dmod
    sys.modules["tensorflow"] = mod
    sys.modules["tensorflow.keras"] = kmod
    sys.modules["tensorflow.keras.optimizers"] = omod
    sys.modules["tensorflow.keras.metrics"] = mmod
    sys.modules["tensorflow.data"] = dmod
    return True


def install_openrec_alias():
    """`openrec.tf2.*` -> `openrec_amd.tf2.*` (same class names and signatures), unless a real
    `openrec` package is importable."""
    import importlib
    import importlib.util
    if "openrec" in sys.modules and getattr(sys.modules["openrec"], "__openrec_amd_alias__", False):
        return True
    try:
        if importlib.util.find_spec("openrec") is not None:
            return False
    except (ImportError, ValueError):
        pass
    top = types.ModuleType("openrec")
    top.__openrec_amd_alias__ = True
    top.__path__ = []
    tf2 = importlib.import_module("openrec_amd.tf2")
    sys.modules["openrec"] = top
    sys.modules["openrec.tf2"] = tf2
    top.tf2 = tf2
    for sub in ("data", "recommenders", "metrics", "modules"):
        m = importlib.import_module("openrec_amd.tf2." + sub)
        sys.modules["openrec.tf2." + sub] = m
    return True
