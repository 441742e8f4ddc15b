"""Thin object layer over the C ABI: Context (device + stream), Table (fp32
[rows, dim] in HBM), Optimizer (Keras sparse-apply rules), and the fused train
steps.  Host-side plumbing only; all arithmetic runs in libopenrec_hip.so."""
from __future__ import annotations

import ctypes
import weakref
from ctypes import byref, c_double, c_int32, c_int64, c_void_p

import os

import numpy as np

from . import _ffi
from ._ffi import check

_default_ctx = None


def _is_device_tensor(x):
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


class DevicePtr:
    """A raw device pointer + element count (ids already resident in HBM)."""

    def __init__(self, ptr, n, keepalive=None):
        self.ptr, self.n, self.keepalive = int(ptr), int(n), keepalive


def _ids_arg(x):
    """-> (pointer, n, on_device, keepalive)"""
    if isinstance(x, DevicePtr):
        return x.ptr, x.n, True, x
    if _is_device_tensor(x):
        assert str(x.dtype).endswith("int32"), "device ids must be int32"
        assert x.is_contiguous()
        return x.data_ptr(), x.numel(), True, x
    if hasattr(x, "numpy") and not isinstance(x, np.ndarray):      # lazy / cpu tensors
        x = x.numpy()
    a = np.ascontiguousarray(x, dtype=np.int32).reshape(-1)       # tf.cast(ids, int32) in Embedding.call
    return a.ctypes.data, a.size, False, a


def _label_arg(x):
    """a float32 list -> (pointer, n, on_device, keepalive)"""
    if _is_device_tensor(x):
        assert str(x.dtype).endswith("float32") and x.is_contiguous()
        return x.data_ptr(), x.numel(), True, x
    if hasattr(x, "numpy") and not isinstance(x, np.ndarray):
        x = x.numpy()
    a = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    return a.ctypes.data, a.size, False, a


class Context:
    def __init__(self, device=0, stream=None):
        self._lib = _ffi.load()
        h = c_void_p()
        check(self._lib.orx_ctx_create(int(device), c_void_p(stream) if stream else None, byref(h)))
        self._h = h
        self.device = int(device)
        self._fin = weakref.finalize(self, self._lib.orx_ctx_destroy, h)

    def synchronize(self):
        check(self._lib.orx_synchronize(self._h))

    def wait_stream(self, stream_handle):
        """later calls on this context wait for the work `stream_handle` (a hipStream_t as int; 0 = default stream) holds now"""
        check(self._lib.orx_ctx_wait_stream(self._h, c_void_p(int(stream_handle)) if stream_handle else None))

    def after_torch(self, *tensors):
        """device tensors produced by torch ops are read by the library on ITS stream: order it behind torch's current one"""
        for t in tensors:
            if _is_device_tensor(t):
                import torch
                self.wait_stream(torch.cuda.current_stream(t.device).cuda_stream)
                return

    def check_index_error(self):
        check(self._lib.orx_check_index_error(self._h))

    # ---- kernel-time sampling ------------------------------------------
    def prof_enable(self, on=True):
        check(self._lib.orx_prof_enable(self._h, 1 if on else 0))

    def prof_reset(self):
        check(self._lib.orx_prof_reset(self._h))

    def stat(self, what):
        """orx_ctx_stat: 'pairs' | 'max_dup' | 'nowait_calls' | 'quiet' of the most recent exact pairwise call's plan"""
        v = c_int64()
        check(self._lib.orx_ctx_stat(self._h, {"pairs": 0, "max_dup": 1, "nowait_calls": 2, "quiet": 3}[what], byref(v)))
        return int(v.value)

    def copy_bandwidth(self, nbytes=1 << 30, reps=10):
        """orx_copy_bandwidth: GB/s (read + write) of a float4 streaming copy over two buffers of `nbytes` each"""
        v = c_double()
        check(self._lib.orx_copy_bandwidth(self._h, int(nbytes), int(reps), byref(v)))
        return float(v.value)

    def prof_get(self):
        out = {}
        for kid, name in _ffi.KERNEL_NAMES.items():
            ms, n = c_double(), c_int64()
            check(self._lib.orx_prof_get(self._h, kid, byref(ms), byref(n)))
            out[name] = dict(total_ms=ms.value, launches=n.value)
        return out


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class Table:
    """fp32 [rows, dim] embedding table resident in HBM."""

    def __init__(self, rows, dim, ctx=None, device_ptr=None, keepalive=None):
        self.ctx = ctx or default_context()
        self._lib = self.ctx._lib
        h = c_void_p()
        if device_ptr is None:
            check(self._lib.orx_table_create(self.ctx._h, int(rows), int(dim), byref(h)))
        else:
            check(self._lib.orx_table_wrap(self.ctx._h, c_void_p(int(device_ptr)), int(rows), int(dim), byref(h)))
        self._h = h
        self.rows, self.dim = int(rows), int(dim)
        self._keepalive = (keepalive, self.ctx)
        self._fin = weakref.finalize(self, self._lib.orx_table_destroy, h)
        self.pre_access = None          # callable run before any host-visible access (queued train steps flush here)

    pre_access = None

    def _sync_pending(self):
        if self.pre_access is not None:
            self.pre_access()

    @property
    def shape(self):
        return (self.rows, self.dim)

    @property
    def device_ptr(self):
        return self._lib.orx_table_device_ptr(self._h)

    def init_uniform(self, lo=-0.05, hi=0.05, seed=0):
        self._sync_pending()
        check(self._lib.orx_table_init_uniform(self._h, lo, hi, int(seed) & (2 ** 64 - 1)))
        return self

    def fill(self, v):
        self._sync_pending()
        check(self._lib.orx_table_fill(self._h, float(v)))
        return self

    def read(self, row0=0, nrows=None):
        self._sync_pending()
        nrows = self.rows - row0 if nrows is None else nrows
        out = np.empty((nrows, self.dim), np.float32)
        check(self._lib.orx_table_read(self._h, int(row0), int(nrows), out.ctypes.data))
        return out

    def numpy(self):
        return self.read()

    def write(self, values, row0=0):
        self._sync_pending()
        a = np.ascontiguousarray(values, np.float32).reshape(-1, self.dim)
        check(self._lib.orx_table_write(self._h, int(row0), a.shape[0], a.ctypes.data))
        return self

    def gather(self, ids):
        self._sync_pending()
        ptr, n, dev, keep = _ids_arg(ids)
        if dev:
            raise ValueError("Table.gather returns host rows; pass host ids (use gather_rows for device buffers)")
        out = np.empty((n, self.dim), np.float32)
        check(self._lib.orx_table_gather(self._h, ptr, n, out.ctypes.data, 0))
        return out

    def censor(self, ids, min_norm=0.1):
        self._sync_pending()
        ptr, n, dev, keep = _ids_arg(ids)
        check(self._lib.orx_table_censor(self._h, ptr, n, float(min_norm), _ffi.ORX_IDS_DEVICE if dev else 0))


class Optimizer:
    KINDS = {"sgd": _ffi.ORX_SGD, "adagrad": _ffi.ORX_ADAGRAD, "adam": _ffi.ORX_ADAM, "momentum": _ffi.ORX_MOMENTUM}
    NSLOTS = {"sgd": 0, "adagrad": 1, "adam": 2, "momentum": 1}

    def __init__(self, kind, lr, p0=0.0, p1=0.0, p2=0.0, ctx=None):
        self.ctx = ctx or default_context()
        self._lib = self.ctx._lib
        self.kind = kind
        self.params = (float(p0), float(p1), float(p2))
        h = c_void_p()
        check(self._lib.orx_opt_create(self.ctx._h, self.KINDS[kind], lr, p0, p1, p2, byref(h)))
        self._h = h
        self._tables = []          # keep tables alive while the optimizer holds slots for them
        self._fin = weakref.finalize(self, self._lib.orx_opt_destroy, h)

    @classmethod
    def sgd(cls, lr=0.01, ctx=None):
        return cls("sgd", lr, ctx=ctx)

    @classmethod
    def adagrad(cls, lr=0.001, initial_accumulator_value=0.1, epsilon=1e-7, ctx=None):
        return cls("adagrad", lr, initial_accumulator_value, epsilon, ctx=ctx)

    @classmethod
    def adam(cls, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, ctx=None):
        return cls("adam", lr, beta_1, beta_2, epsilon, ctx=ctx)

    @classmethod
    def momentum(cls, lr=0.01, momentum=0.9, nesterov=False, ctx=None):
        """keras.optimizers.SGD(lr, momentum, nesterov): slot 0 is the velocity (Keras' "momentum" slot)"""
        return cls("momentum", lr, momentum, 1.0 if nesterov else 0.0, ctx=ctx)

    def set_lr(self, lr):
        check(self._lib.orx_opt_set_lr(self._h, lr))

    @property
    def step(self):
        """the step counter (Keras `optimizer.iterations`)"""
        t = c_int64(0)
        check(self._lib.orx_opt_get_step(self._h, byref(t)))
        return int(t.value)

    @step.setter
    def step(self, value):
        check(self._lib.orx_opt_set_step(self._h, int(value)))

    def advance(self, tables=None):
        """One optimizer step begins (Keras `iterations` += 1) for a host that applies gradients through `apply_rows`.
        `tables`: the tables this step updates -- any other table lazily applied under this optimizer is finished first
        and takes no Adam decay for the step (Keras updates only the variables handed to apply_gradients); None: the
        optimizer's own tables, all of them."""
        if tables is None:
            check(self._lib.orx_opt_advance(self._h, None, -1))
        else:
            arr = (c_void_p * len(tables))(*[t._h for t in tables])
            check(self._lib.orx_opt_advance(self._h, ctypes.cast(arr, c_void_p), len(tables)))

    def slot(self, table, slot=0):
        out = np.empty((table.rows, table.dim), np.float32)
        check(self._lib.orx_opt_slot_read(self._h, table._h, slot, 0, table.rows, out.ctypes.data))
        return out

    def set_slot(self, table, values, slot=0):
        a = np.ascontiguousarray(values, np.float32).reshape(table.rows, table.dim)
        check(self._lib.orx_opt_slot_write(self._h, table._h, slot, 0, table.rows, a.ctypes.data))

    def slot_rows(self, table, slot, row0, nrows):
        """rows [row0, row0 + nrows) of an optimizer slot of `table` (checkpoints stream slots in row ranges)"""
        out = np.empty((nrows, table.dim), np.float32)
        check(self._lib.orx_opt_slot_read(self._h, table._h, int(slot), int(row0), int(nrows), out.ctypes.data))
        return out

    def set_slot_rows(self, table, values, slot, row0):
        a = np.ascontiguousarray(values, np.float32).reshape(-1, table.dim)
        check(self._lib.orx_opt_slot_write(self._h, table._h, int(slot), int(row0), a.shape[0], a.ctypes.data))


def _bias_h(bias):
    """the C handle of an optional item-bias table (None: a model without item biases -- bias-free BPR)"""
    return None if bias is None else bias._h


def _keep_tables(opt, tables):
    """the optimizer keeps the tables it holds slots for alive (never None)"""
    opt._tables = list({id(t): t for t in (opt._tables + [t for t in tables if t is not None])}.values())


_TRAIN_ROLES = {"user": _ffi.ORX_TRAIN_USER, "item": _ffi.ORX_TRAIN_ITEM, "bias": _ffi.ORX_TRAIN_BIAS}
_MN_KIND = {"softmax": _ffi.ORX_MN_SOFTMAX, "logsig": _ffi.ORX_MN_LOGSIG}


# ---- the argument layer of the train-step and forward-loss calls ---------------------------------------------------
# Every step / loss entry point below reads its arguments through these functions, each check written once.  The order of
# refusals is the same everywhere: `train` and the coefficients first (_mask_arg, _coef_arg, _l2_arg: no table, optimizer or
# context is touched), then the family's own bounds and _dot_tables (shapes only), then the lists (_list_args or its parts:
# sides, K / B / id_stride, lengths), and only then the context -- after_torch for every device buffer handed over, the
# tables' _sync_pending where the family flushes, `_lib`.  Every refusal is a ValueError that names the call.
def _mask_arg(what, train, roles, has_bias):
    """`train` of a step -> the OR of the named tables' bits in `roles` (a family's role dictionary), or None for train=None:
    every table.  A name or an iterable of names: the tables that receive the step's updates; every other table is read,
    never written."""
    if train is None:
        return None
    names = [train] if isinstance(train, str) else list(train)
    unknown = [r for r in names if r not in roles]
    if unknown:
        raise ValueError(f"{what}: train: unknown table name(s) {unknown!r}; expected a subset of {sorted(roles)}")
    if not names:
        raise ValueError(f"{what}: train: empty set (no table would be trained); pass None to train every table")
    if "bias" in names and not has_bias:
        raise ValueError(f'{what}: train: "bias" named, but the model has no item-bias table (bias=None)')
    mask = 0
    for r in names:
        mask |= roles[r]
    return mask


def _train_mask(train, bias, what="step"):
    """`train` of the user / item / bias steps -> orx_train_mask, or None for the full step"""
    return _mask_arg(what, train, _TRAIN_ROLES, bias is not None)


def _coef_arg(what, name, x):
    """a coefficient of the objective (l2_reg, l2_proj) -> a float that is finite and >= 0"""
    x = float(x)
    if not (np.isfinite(x) and x >= 0.0):
        raise ValueError(f"{what}: {name} must be finite and >= 0 (got {x})")
    return x


def _l2_arg(what, l2_reg, no_l2, default_is_one=False):
    """l2_reg (None: 1) and no_l2 (the coefficient 0) of a step -> the coefficient of l2_loss.  no_l2 goes with no l2_reg of the
    caller's own: None, and where the step's signature defaults l2_reg to 1.0 (default_is_one) also that value and 0."""
    if no_l2:
        if l2_reg is not None and not (default_is_one and l2_reg in (0, 0.0, 1.0)):
            raise ValueError(f"{what}: no_l2=True together with l2_reg = {l2_reg} (drop no_l2, or pass l2_reg=0.0)")
        return 0.0
    return _coef_arg(what, "l2_reg", 1.0 if l2_reg is None else l2_reg)


def _negatives_arg(what, loss, nid, exact=False):
    """the loss kind and the negatives of an N-negatives call -> (orx_multineg_kind, N); N is nid's last axis, nid shaped
    [..., B, N] (exact: [B, N] and nothing in front)"""
    if loss not in _MN_KIND:
        raise ValueError(f"{what}: unknown loss {loss!r}; expected one of {sorted(_MN_KIND)}")
    shape = tuple(getattr(nid, "shape", ()))
    if isinstance(nid, DevicePtr) or (len(shape) != 2 if exact else len(shape) < 2):
        raise ValueError(f"{what}: nid must be an array shaped [{'' if exact else '..., '}B, N] (N is taken from its last axis)")
    N = int(shape[-1])
    if not 1 <= N <= 64:
        raise ValueError(f"{what}: N = {N} negatives per positive; N must be in [1, 64]")
    return _MN_KIND[loss], N


def _dot_tables(what, user_dim, item_dim, items, bias):
    """the tables of a dot-product family (shapes only): the user side's dim is the item side's, the bias is [items, 1] or None"""
    if user_dim != item_dim:
        raise ValueError(f"{what}: user dim {user_dim} != item dim {item_dim} (dot scores only)")
    if bias is not None and tuple(bias.shape) != (items, 1):
        raise ValueError(f"{what}: bias must be [{items}, 1], got {list(bias.shape)}")


def _id_lists(what, lists, dev=None):
    """the id lists of a call, all on one side (dev: the side something else of the call has settled already)
    -> (pointers, lengths, on_device, keepalives)"""
    ptrs, ns, keep = [], [], []
    for x in lists:
        p, n, d, k = _ids_arg(x)
        if dev is None:
            dev = d
        elif d != dev:
            raise ValueError(f"{what}: ids must be all on the host or all on the device")
        ptrs.append(p); ns.append(n); keep.append(k)
    return ptrs, ns, dev, keep


def _floats_arg(what, name, x, ids_on_device, n, like):
    """a float32 list beside the ids (label, weights, neg_offset, item_offset; None: absent) -> (pointer, keepalive); it lives
    where the ids live and has n elements, shaped like the list `like`"""
    if x is None:
        return None, None
    p, nx, dx, k = _label_arg(x)
    if dx != ids_on_device:
        raise ValueError(f"{what}: {name} on the {'device' if dx else 'host'} with ids on the {'device' if ids_on_device else 'host'} "
                         f"({name} lives where the ids live)")
    if nx != n:
        raise ValueError(f"{what}: {nx} {name} for {n} ids ({name} is shaped like {like})")
    return p, k


def _step_shape(what, K, B, id_stride, n_ids, overlap=False):
    """K, B and id_stride of a K-step call over id lists of n_ids elements (B None: n_ids // K; id_stride None: B) -> the three
    as ints and the elements a list needs.  id_stride >= B, as the C side of the dot-product families has it; overlap (the
    pairwise and pointwise steps, whose C side takes any stride): steps may share ids, down to id_stride = 0 for one batch K
    times, and only a stride that would step in front of the lists is refused (K = 1 never looks at it)."""
    K = int(K)
    if K < 0:
        raise ValueError(f"{what}: K = {K}")
    if B is None:
        B = n_ids // K if K else 0
    B = int(B)
    if id_stride is None:
        id_stride = B
    id_stride = int(id_stride)
    if B < 0 or (id_stride < 0 and K > 1 if overlap else id_stride < B):
        raise ValueError(f"{what}: B = {B}, id_stride = {id_stride} (id_stride >= {'0' if overlap else 'B'}, B >= 0)")
    return K, B, id_stride, ((K - 1) * id_stride + B if K and B else 0)


def _loss_outputs(K, want_loss):
    """-> ((loss[K], l2[K]) as numpy float32 or None, and the two pointers for the library)"""
    if not want_loss:
        return None, None, None
    out = np.empty(K, np.float32), np.empty(K, np.float32)
    return out, out[0].ctypes.data, out[1].ctypes.data


def _loss_pair(out):
    """the (loss, l2) of a forward-only call, written by the library into _loss_outputs(1, True)'s arrays, as two floats"""
    return float(out[0][0]), float(out[1][0])


def _flags(ids_on_device, bits=0):
    """the flag word of a call: ORX_IDS_DEVICE where the lists live on the device, OR-ed with the call's own bits"""
    return bits | _ffi.ORX_IDS_DEVICE if ids_on_device else bits


def _list_args(what, names, ids, floats, K=1, B=None, id_stride=None, N=1, overlap=False):
    """The lists of a K-step call (a forward-only call: K = 1 over the whole lists).  ids: the id lists, called `names`, alike
    in length and the last N times as long; floats: (name, list or None, index of the id list it is shaped like) triples.  All
    live on one side, and every id list holds what K steps of B at id_stride read (overlap: as in _step_shape).
    -> K, B, id_stride, on_device, the pointers (ids, then floats; None for an absent list), the keepalives.  The keepalives
    are the caller's to hold until the library has returned and to hand to after_torch: device tensors are among them as they
    came."""
    ptrs, ns, dev, keep = _id_lists(what, ids)
    n = ns[0]
    K, B, id_stride, need = _step_shape(what, K, B, id_stride, n, overlap)
    if n < need or ns[-1] != n * N or not all(m == n for m in ns[:-1]):
        raise ValueError(f"{what}: " + ", ".join(f"{m} {name}" for name, m in zip(names, ns)) + f" ids for K = {K}, B = {B}, "
                         f"id_stride = {id_stride} (the lists alike{f', {names[-1]} N = {N} times as long' if N != 1 else ''}, "
                         f"at least {need} each)")
    for name, x, like in floats:
        p, k = _floats_arg(what, name, x, dev, ns[like], names[like])
        ptrs.append(p); keep.append(k)
    return K, B, id_stride, dev, ptrs, keep


def _triplet_args(what, uid, pid, nid, weights=None, K=1, B=None, id_stride=None, overlap=False):
    """_list_args of a call over (user, positive, negative) triplets with optional per-triplet weights"""
    return _list_args(what, ("uid", "pid", "nid"), (uid, pid, nid), (("weights", weights, 0),), K, B, id_stride, 1, overlap)


def pairwise_step(model, opt, user, item, bias, uid, pid, nid, K=1, B=None, id_stride=None,
                  margin=0.5, hogwild=False, no_l2=False, want_loss=True, censor=False, train=None,
                  weights=None, l2_reg=None):
    """K fused train steps.  Returns (loss[K], l2[K]) as numpy float32 when
    want_loss, else None (fully asynchronous).  bias=None: BPR without item biases (score u.p - u.n); UCML and
    censor need the bias (ValueError).  train: None, or the tables to update ("user", "item", "bias"); the others stay
    bit-for-bit as they are (orx_pairwise_step_subset).
    weights / l2_reg (orx_pairwise_step_weighted): the objective loss_w + l2_reg * l2_loss, where weights[i] multiplies triplet
    i's term inside BPR's mean / UCML's sum.  weights: a float32 numpy array or device tensor shaped like the ids and living where
    they live; the returned loss is the weighted one, l2 the unscaled l2_loss.  Both None: the plain step, as ever.
    uid / pid / nid: alike in length and on one side, each at least (K - 1) * id_stride + B long (B None: len // K; id_stride
    None: B); K = 0 is the library's no-op.  Bad arguments raise ValueError before the library is called."""
    what = "pairwise_step"
    mask = _train_mask(train, bias, what)
    weighted = weights is not None or l2_reg is not None
    if weighted:
        l2c = _l2_arg(what, l2_reg, no_l2)
    K, B, id_stride, dev, (pu, pp, pn, pw), keep = _triplet_args(what, uid, pid, nid, weights, K, B, id_stride, True)
    user.ctx.after_torch(*keep)
    lib = user.ctx._lib
    flags = _flags(dev, (_ffi.ORX_HOGWILD if hogwild else 0) | (_ffi.ORX_NO_L2 if no_l2 else 0) | (_ffi.ORX_CENSOR if censor else 0))
    mid = {"bpr": _ffi.ORX_BPR, "ucml": _ffi.ORX_UCML}[model]
    out, lp, l2p = _loss_outputs(K, want_loss)
    head = (user.ctx._h, mid, opt._h, user._h, item._h, _bias_h(bias), pu, pp, pn)
    if weighted:
        check(lib.orx_pairwise_step_weighted(*head, pw, K, B, id_stride, float(margin), l2c, flags & ~_ffi.ORX_NO_L2,
                                             mask or 0, lp, l2p))
    elif mask is None:
        check(lib.orx_pairwise_step(*head, K, B, id_stride, float(margin), flags, lp, l2p))
    else:
        check(lib.orx_pairwise_step_subset(*head, K, B, id_stride, float(margin), flags, mask, lp, l2p))
    _keep_tables(opt, (user, item, bias))
    return out


def pairwise_reserve(opt, user, item, bias, K, B):
    """Pre-size every per-call device buffer for calls of up to K steps of B triplets (bias may be None)."""
    check(user.ctx._lib.orx_pairwise_reserve(user.ctx._h, opt._h, user._h, item._h, _bias_h(bias), int(K), int(B)))
    _keep_tables(opt, (user, item, bias))


def pairwise_loss(model, user, item, bias, uid, pid, nid, margin=0.5, weights=None):
    """forward only: (loss, l2_loss) of one batch; weights: per-triplet weights as in pairwise_step"""
    what = "pairwise_loss"
    _, B, _, dev, (pu, pp, pn, pw), keep = _triplet_args(what, uid, pid, nid, weights)
    user.ctx.after_torch(*keep)
    lib = user.ctx._lib
    mid = {"bpr": _ffi.ORX_BPR, "ucml": _ffi.ORX_UCML}[model]
    out, lp, l2p = _loss_outputs(1, True)
    head = (user.ctx._h, mid, user._h, item._h, _bias_h(bias), pu, pp, pn)
    if weights is not None:
        check(lib.orx_pairwise_loss_weighted(*head, pw, B, float(margin), _flags(dev), lp, l2p))
    else:
        check(lib.orx_pairwise_loss(*head, B, float(margin), _flags(dev), lp, l2p))
    return _loss_pair(out)


def _multineg_args(what, loss, user, item, bias, uid, pid, nid, K, B, id_stride, weights, neg_offset):
    """the checks and the pointers multineg_step and multineg_loss share; every bad argument is a ValueError raised here,
    before the library is called"""
    kind, N = _negatives_arg(what, loss, nid)
    _dot_tables(what, user.shape[1], item.shape[1], item.shape[0], bias)
    K, B, id_stride, dev, ptrs, keep = _list_args(what, ("uid", "pid", "nid"), (uid, pid, nid),
                                                  (("weights", weights, 0), ("neg_offset", neg_offset, 2)), K, B, id_stride, N)
    user.ctx.after_torch(*keep)
    return kind, N, K, B, id_stride, dev, ptrs, keep


def multineg_step(loss, opt, user, item, bias, uid, pid, nid, K=1, B=None, id_stride=None, weights=None, neg_offset=None,
                  l2_reg=1.0, no_l2=False, want_loss=True):
    """K train steps of one positive against N negatives per sample (orx_multineg_step).  loss: "softmax" -- sampled softmax,
    -log softmax of the positive among the 1 + N logits -- or "logsig" -- the mean of N BPR log-sigmoid pair terms.  Scores are
    dot products plus the item bias (bias=None: none).  nid is shaped [..., B, N] and N (1 .. 64) is taken from it; uid / pid as
    in pairwise_step.  weights: per-sample weights shaped like uid; neg_offset: a constant added to every negative's logit,
    shaped like nid (-log Q(item) for negatives from a weighted proposal; -inf drops a negative); both live where the ids live.
    The objective is loss + l2_reg * l2_loss (no_l2=True: l2_reg = 0).  Returns (loss[K], l2[K]) as numpy float32 -- l2 the
    unscaled l2_loss -- when want_loss, else None (fully asynchronous).  Bad arguments raise ValueError before the library is
    called; an id outside its table raises IndexError."""
    what = "multineg_step"
    l2c = _l2_arg(what, l2_reg, no_l2, default_is_one=True)
    kind, N, K, B, id_stride, dev, ptrs, keep = _multineg_args(what, loss, user, item, bias, uid, pid, nid, K, B, id_stride,
                                                                weights, neg_offset)
    out, lp, l2p = _loss_outputs(K, want_loss)
    check(user.ctx._lib.orx_multineg_step(user.ctx._h, kind, opt._h, user._h, item._h, _bias_h(bias), *ptrs, K, B, N, id_stride,
                                          l2c, _flags(dev), lp, l2p))
    _keep_tables(opt, (user, item, bias))
    return out


def multineg_loss(loss, user, item, bias, uid, pid, nid, weights=None, neg_offset=None):
    """forward only: (loss, l2_loss) of one batch of multineg_step -- the step's own numbers bit for bit on the same tables; no
    table changes"""
    kind, N, _, B, _, dev, ptrs, keep = _multineg_args("multineg_loss", loss, user, item, bias, uid, pid, nid, 1, None, None,
                                                       weights, neg_offset)
    out, lp, l2p = _loss_outputs(1, True)
    check(user.ctx._lib.orx_multineg_loss(user.ctx._h, kind, user._h, item._h, _bias_h(bias), *ptrs, B, N, _flags(dev), lp, l2p))
    return _loss_pair(out)


def _inbatch_args(what, user, item, bias, uid, pid, K, B, id_stride, weights, item_offset, scale, chunk):
    """the checks and the pointers inbatch_step and inbatch_loss share; every bad argument is a ValueError raised here, before
    the library is called"""
    _dot_tables(what, user.shape[1], item.shape[1], item.shape[0], bias)
    if user.shape[1] > 256:
        raise ValueError(f"{what}: dim {user.shape[1]} above 256")
    scale = float(scale)
    if not (np.isfinite(scale) and scale > 0.0):
        raise ValueError(f"{what}: scale must be finite and > 0 (got {scale})")
    chunk = int(chunk)
    if chunk < 0 or chunk % 64:
        raise ValueError(f"{what}: chunk = {chunk}; 0 (the launcher's choice) or a multiple of the tile width 64")
    K, B, id_stride, dev, ptrs, keep = _list_args(what, ("uid", "pid"), (uid, pid),
                                                  (("weights", weights, 0), ("item_offset", item_offset, 1)), K, B, id_stride)
    user.ctx.after_torch(*keep)
    return K, B, id_stride, dev, ptrs, scale, chunk, keep


def inbatch_step(opt, user, item, bias, uid, pid, K=1, B=None, id_stride=None, weights=None, item_offset=None, scale=1.0,
                 mask_hits=True, l2_reg=1.0, no_l2=False, want_loss=True, chunk=0):
    """K train steps on in-batch negatives (orx_inbatch_step): the positive of every sample is scored against the positives of
    all B samples of its step, s_ij = scale (u_i . v_j + b_j) + off_j, and the loss is the softmax over the row -- no sampler, no
    B x B matrix.  uid / pid as in pairwise_step; bias=None: no item bias.  weights: per-sample weights; item_offset: added to
    column j in every row (-log Q(pid[j]) is the log-Q correction); both shaped like the ids and living where they live.
    scale = 1 / temperature.  mask_hits: a column with the row's own positive item (other than the diagonal) is no negative.
    The objective is loss + l2_reg * l2_loss (no_l2=True: l2_reg = 0).  chunk: columns per chunk of a row block, 0 for the
    launcher's choice.  Returns (loss[K], l2[K]) as numpy float32 -- l2 the unscaled l2_loss -- when want_loss, else None
    (fully asynchronous).  Bad arguments raise ValueError before the library is called; an id outside its table IndexError."""
    what = "inbatch_step"
    l2c = _l2_arg(what, l2_reg, no_l2, default_is_one=True)
    K, B, id_stride, dev, ptrs, scale, chunk, keep = _inbatch_args(what, user, item, bias, uid, pid, K, B, id_stride, weights,
                                                                   item_offset, scale, chunk)
    out, lp, l2p = _loss_outputs(K, want_loss)
    flags = _flags(dev, (_ffi.ORX_IB_MASK_HITS if mask_hits else 0) | (_ffi.ORX_NO_L2 if no_l2 else 0))
    check(user.ctx._lib.orx_inbatch_step(user.ctx._h, opt._h, user._h, item._h, _bias_h(bias), *ptrs, K, B, id_stride, scale, l2c,
                                         chunk, flags, lp, l2p))
    _keep_tables(opt, (user, item, bias))
    return out


def inbatch_loss(user, item, bias, uid, pid, weights=None, item_offset=None, scale=1.0, mask_hits=True, chunk=0, per_row=False):
    """forward only: (loss, l2_loss) of one batch of inbatch_step -- the step's own numbers bit for bit on the same tables; no
    table changes.  per_row=True: (loss, l2_loss, l) with l_i of every sample, a numpy float32 array [B]"""
    _, B, _, dev, ptrs, scale, chunk, keep = _inbatch_args("inbatch_loss", user, item, bias, uid, pid, 1, None, None, weights,
                                                           item_offset, scale, chunk)
    out, lp, l2p = _loss_outputs(1, True)
    rows, rp = _row_loss_buffer(user.ctx, B, dev, per_row)
    flags = _flags(dev, _ffi.ORX_IB_MASK_HITS if mask_hits else 0)
    check(user.ctx._lib.orx_inbatch_loss(user.ctx._h, user._h, item._h, _bias_h(bias), *ptrs, B, scale, chunk, flags, lp, l2p, rp))
    return _forward_result(out, rows, dev)


def inbatch_geometry(B, D, chunk=0):
    """what the launcher of inbatch_step does for (B, D, chunk): a dict of own rows per workgroup, columns per tile, column
    chunks per row block and the padded dim.  No device is needed."""
    out = (c_int32 * 4)()
    check(_ffi.load().orx_inbatch_geometry(int(B), int(D), int(chunk), out))
    return dict(rows=int(out[0]), tile=int(out[1]), chunks=int(out[2]), dim=int(out[3]))


# ---- the full softmax over all items (orx_fullsoftmax_step / orx_fullsoftmax_loss; SeqRec.step_full is the pooled-query form) ----
def _chunk_arg(what, name, x):
    """chunk_items / chunk_samples -> an int that is 0 (the launcher's choice) or a positive multiple of the tile width 64"""
    x = int(x)
    if x < 0 or x % 64:
        raise ValueError(f"{what}: {name} = {x}; 0 (the launcher's choice) or a multiple of the tile width 64")
    return x


def _scale_arg(what, scale):
    scale = float(scale)
    if not (np.isfinite(scale) and scale > 0.0):
        raise ValueError(f"{what}: scale must be finite and > 0 (got {scale})")
    return scale


def _fullsoftmax_args(what, user, item, bias, uid, pid, weights, item_offset, scale, chunk_items, chunk_samples):
    """the checks and the pointers fullsoftmax_step and fullsoftmax_loss share; every bad argument is a ValueError raised
    here, before the library is called"""
    _dot_tables(what, user.shape[1], item.shape[1], item.shape[0], bias)
    if user.shape[1] > 256:
        raise ValueError(f"{what}: dim {user.shape[1]} above 256")
    scale = _scale_arg(what, scale)
    ci, cs = _chunk_arg(what, "chunk_items", chunk_items), _chunk_arg(what, "chunk_samples", chunk_samples)
    _, B, _, dev, (pu, pp, pw), keep = _list_args(what, ("uid", "pid"), (uid, pid), (("weights", weights, 0),))
    if B >= 2 ** 31 - 256 or item.shape[0] >= 2 ** 31 - 256:
        raise ValueError(f"{what}: B = {B} samples, {item.shape[0]} items; both must fit 31 bits")
    po, ko = _floats_arg(what, "item_offset", item_offset, dev, item.shape[0], "the item table's rows")      # one float per ITEM
    user.ctx.after_torch(*keep, ko)
    return B, dev, (pu, pp, pw, po), scale, ci, cs, (keep, ko)


def fullsoftmax_step(opt, user, item, bias, uid, pid, weights=None, item_offset=None, scale=1.0, l2_reg=0.0, train=None,
                     chunk_items=0, chunk_samples=0, want_loss=True):
    """One train step on the softmax over ALL items (orx_fullsoftmax_step): sample i's label pid[i] against every row of the
    item table, s_ij = scale (u_i . V[j] + b[j]) + off[j] with u_i = user[uid[i]] -- the reference's
    sparse_softmax_cross_entropy_with_logits over a Dense(total_items) -- without a B x items matrix.  bias=None: no item bias.
    weights: per-sample weights shaped like the ids; item_offset: one float per ITEM ([items]; a log-prior, -inf removes the
    item from every softmax); both live where the ids live.  The objective is loss + l2_reg * l2_loss, l2_loss over the 2B
    looked-up rows.  The user table takes the sparse rule on uid, the item table and the bias the optimizer's dense rule on
    every row.  train: None, or a subset of ("user", "item", "bias") -- every other table is read, never written.
    chunk_items / chunk_samples: 0 for the launcher's choice, or multiples of 64.  Returns (loss[1], l2[1]) as numpy float32
    -- l2 the unscaled l2_loss -- when want_loss, else None (device ids: no host synchronisation).  Bad arguments raise
    ValueError before the library is called; an id outside its table IndexError."""
    what = "fullsoftmax_step"
    mask = _train_mask(train, bias, what) or 0
    l2c = _coef_arg(what, "l2_reg", l2_reg)
    B, dev, ptrs, scale, ci, cs, keep = _fullsoftmax_args(what, user, item, bias, uid, pid, weights, item_offset, scale,
                                                           chunk_items, chunk_samples)
    out, lp, l2p = _loss_outputs(1, want_loss)
    check(user.ctx._lib.orx_fullsoftmax_step(user.ctx._h, opt._h, user._h, item._h, _bias_h(bias), *ptrs, B, scale, l2c, ci, cs,
                                             mask, _flags(dev), lp, l2p))
    _keep_tables(opt, (user, item, bias))
    return out


def _row_loss_buffer(ctx, B, dev, per_row):
    """the [B] output of a forward's row losses where the ids live -> (array or tensor or None, pointer or None)"""
    if not per_row:
        return None, None
    if dev:
        import torch
        rows = torch.empty(B, dtype=torch.float32, device=torch.device("cuda", ctx.device))
        ctx.after_torch(rows)
        return rows, rows.data_ptr()
    rows = np.empty(B, np.float32)
    return rows, rows.ctypes.data


def _forward_result(out, rows, dev):
    """what a forward-only call returns: (loss, l2_loss), and with _row_loss_buffer's rows (loss, l2_loss, l) as numpy"""
    if rows is None:
        return _loss_pair(out)
    if dev:
        rows = rows.cpu().numpy()          # (the call has synchronised the context's stream for the two sums)
    return (*_loss_pair(out), rows)


def fullsoftmax_loss(user, item, bias, uid, pid, weights=None, item_offset=None, scale=1.0, chunk_items=0, per_row=False):
    """forward only: (loss, l2_loss) of one batch of fullsoftmax_step -- the step's own numbers bit for bit on the same tables;
    no table changes.  per_row=True: (loss, l2_loss, l) with l_i of every sample, a numpy float32 array [B]"""
    what = "fullsoftmax_loss"
    B, dev, ptrs, scale, ci, _, keep = _fullsoftmax_args(what, user, item, bias, uid, pid, weights, item_offset, scale, chunk_items, 0)
    out, lp, l2p = _loss_outputs(1, True)
    rows, rp = _row_loss_buffer(user.ctx, B, dev, per_row)
    check(user.ctx._lib.orx_fullsoftmax_loss(user.ctx._h, user._h, item._h, _bias_h(bias), *ptrs, B, scale, ci, _flags(dev), lp, l2p, rp))
    return _forward_result(out, rows, dev)


def fullsoftmax_geometry(B, items, D, chunk_items=0, chunk_samples=0):
    """what the launcher of fullsoftmax_step does for (B, items, D) and the chunk arguments: a dict of own rows per workgroup,
    rows per tile, item chunks, sample chunks, the padded dim and the scratch bytes of a step.  No device is needed."""
    out = (c_int64 * 6)()
    check(_ffi.load().orx_fullsoftmax_geometry(int(B), int(items), int(D), int(chunk_items), int(chunk_samples), out))
    return dict(rows=int(out[0]), tile=int(out[1]), item_chunks=int(out[2]), sample_chunks=int(out[3]), dim=int(out[4]),
                scratch_bytes=int(out[5]))


_POINT = {"gmf": _ffi.ORX_GMF, "wrmf": _ffi.ORX_WRMF}


def pointwise_step(model, opt, user, item, bias, w, uid, iid, label, K=1, B=None, id_stride=None,
                   a=1.0, b_w=1.0, hogwild=False, no_l2=False, want_loss=True, sigmoid=False, train=None, l2_reg=None):
    """K fused GMF / WRMF train steps (gmf.py:22-34, wrmf.py:21-34); sigmoid: PointwiseMSELoss(sigmoid=True)
    (pointwise_mse_loss.py:24-25; WRMF only).  train: as in pairwise_step (WRMF; GMF takes the full set only).
    l2_reg: the objective loss + l2_reg * l2_loss (orx_pointwise_step_l2reg); the returned l2 stays the unscaled l2_loss.
    uid / iid / label (float32): alike in length and on one side, each at least (K - 1) * id_stride + B long (B None:
    len // K; id_stride None: B); K = 0 is the library's no-op.  Bad arguments raise ValueError before the library is called."""
    what = "pointwise_step"
    mask = _train_mask(train, bias, what)
    if l2_reg is not None:
        l2c = _l2_arg(what, l2_reg, no_l2)
    K, B, id_stride, dev, (pu, pi, pl), keep = _list_args(what, ("uid", "iid"), (uid, iid), (("label", label, 0),), K, B, id_stride, 1, True)
    user.ctx.after_torch(*keep)
    lib = user.ctx._lib
    flags = _flags(dev, (_ffi.ORX_HOGWILD if hogwild else 0) | (_ffi.ORX_NO_L2 if no_l2 else 0)
                   | (_ffi.ORX_POINT_SIGMOID if sigmoid else 0))
    out, *outs = _loss_outputs(K, want_loss)
    args = (user.ctx._h, _POINT[model], opt._h, user._h, item._h, bias._h, w._h if w is not None else None, pu, pi, pl,
            K, B, id_stride, float(a), float(b_w), flags)
    if l2_reg is not None:
        check(lib.orx_pointwise_step_l2reg(*args[:-1], l2c, flags & ~_ffi.ORX_NO_L2, mask or 0, *outs))
    elif mask is None:
        check(lib.orx_pointwise_step(*args, *outs))
    else:
        check(lib.orx_pointwise_step_subset(*args, mask, *outs))
    _keep_tables(opt, (user, item, bias, w))
    return out


def pointwise_loss(model, user, item, bias, w, uid, iid, label, a=1.0, b_w=1.0, sigmoid=False):
    """forward only: (loss, l2_loss) of one batch of pointwise_step"""
    what = "pointwise_loss"
    _, B, _, dev, (pu, pi, pl), keep = _list_args(what, ("uid", "iid"), (uid, iid), (("label", label, 0),))
    user.ctx.after_torch(*keep)
    out, lp, l2p = _loss_outputs(1, True)
    check(user.ctx._lib.orx_pointwise_loss(user.ctx._h, _POINT[model], user._h, item._h, bias._h, w._h if w is not None else None,
                                           pu, pi, pl, B, float(a), float(b_w),
                                           _flags(dev, _ffi.ORX_POINT_SIGMOID if sigmoid else 0), lp, l2p))
    return _loss_pair(out)


class _HostView(np.lib.mixins.NDArrayOperatorsMixin):
    """An array kept in another form (device memory, item lists) that turns into its NumPy value when someone looks:
    `np.asarray(x)`, `x.numpy()`, indexing, arithmetic and any ndarray attribute all go through `_dense()`."""
    _host = None

    def numpy(self):
        if self._host is None:
            self._host = self._dense()
        return self._host

    def __array__(self, dtype=None, copy=None):
        a = self.numpy()
        return a if dtype is None else a.astype(dtype, copy=False)

    def __array_ufunc__(self, ufunc, method, *inputs, **kw):
        return getattr(ufunc, method)(*[x.numpy() if isinstance(x, _HostView) else x for x in inputs], **kw)

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, i):
        return self.numpy()[i]

    def __iter__(self):
        return iter(self.numpy())

    def __getattr__(self, name):                       # (only reached for what the class does not define)
        if name.startswith("__"):
            raise AttributeError(name)
        return getattr(self.numpy(), name)

    ndim = 2


class DeviceScores(_HostView):
    """[n, items] fp32 scores of `Recommender.inference` held in device memory (a torch tensor).  The metrics read them there;
    the host copy (4 bytes x n x items over PCIe) is made only if the script looks at the values."""
    dtype = np.dtype(np.float32)

    def __init__(self, ctx, tensor):
        self.ctx, self.tensor, self.shape = ctx, tensor, tuple(tensor.shape)

    def _dense(self):
        return self.tensor.cpu().numpy()


class _ItemLists:
    """One list of item ids per row over `n_items` items: `ptr` int64 [n + 1] from 0, `items` int32, `shape` (n, n_items)."""

    def __init__(self, ptr, items, n_items):
        self.ptr = np.ascontiguousarray(ptr, np.int64); self.items = np.ascontiguousarray(items, np.int32)
        self.shape = (self.ptr.size - 1, int(n_items))

    def row(self, q):
        return self.items[self.ptr[q]:self.ptr[q + 1]]


class SparseMask(_ItemLists, _HostView):
    """A batch of boolean item masks [n, items] as one sorted list of distinct items per row (CSR): what
    `Dataset.evaluation` hands out instead of the dense rows of openrec/tf2/data/dataset.py:60-82.  Dense on demand."""
    dtype = np.dtype(bool)

    @classmethod
    def from_lists(cls, lists, n_items):
        rows = [np.unique(np.asarray(r, np.int64)) for r in lists]
        for r in rows:
            if r.size and (r[0] < 0 or r[-1] >= n_items):
                raise IndexError(f"item id outside [0, {n_items})")
        ptr = np.zeros(len(rows) + 1, np.int64); np.cumsum([r.size for r in rows], out=ptr[1:])
        return cls(ptr, np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32), n_items)

    @classmethod
    def from_dense(cls, mask):
        m = np.asarray(mask).astype(bool)
        r, c = np.nonzero(m)
        ptr = np.zeros(m.shape[0] + 1, np.int64); np.cumsum(np.bincount(r, minlength=m.shape[0]), out=ptr[1:])
        return cls(ptr, c.astype(np.int32), m.shape[1])

    def _dense(self):
        m = np.zeros(self.shape, bool)
        m[np.repeat(np.arange(self.shape[0]), np.diff(self.ptr)), self.items] = True
        return m


def _kind_arg(kind):
    return {"dot": 0, "l2": 1, "gmf": 2}[kind]


def _scorer_head(user, item, bias, w):
    """the table handles of a scorer call: user, item, bias (None: no "+ b"), GMF's w"""
    return user._h, item._h, _bias_h(bias), w._h if w is not None else None


def _host_uid(what, uid, n=None):
    """host user ids -> (pointer, count, the array to keep alive); `n`: the rows of the masks they go with"""
    ptr, nn, dev, keep = _ids_arg(uid)
    if dev:
        raise ValueError(f"{what} takes host ids")
    if n is not None and nn != n:
        raise ValueError(f"{nn} user ids for masks of {n} rows")
    return ptr, nn, keep


def _metric_outputs(n, at):
    """-> (cut-offs float32 [nat], auc [n], ndcg [n, nat], recall [n, nat], the dict of the three a metrics call returns)"""
    atv = np.ascontiguousarray(at, np.float32).reshape(-1)
    auc = np.empty(n, np.float32); ndcg = np.empty((n, atv.size), np.float32); rec = np.empty((n, atv.size), np.float32)
    return atv, auc, ndcg, rec, dict(auc=auc, ndcg=ndcg, recall=rec)


def score_all_items(kind, user, item, bias, uid, w=None, device=False):
    """Recommender.inference: scores of the given users against ALL items -> [n, item_rows] (host array, or with
    `device=True` a DeviceScores that stays in HBM until someone reads it).  bias=None: no "+ b" (bias-free models)."""
    lib = user.ctx._lib
    ptr, n, keep = _host_uid("score_all_items", uid)
    head = (user.ctx._h, _kind_arg(kind), *_scorer_head(user, item, bias, w), ptr, n)
    if device:
        try:
            import torch
        except ImportError:                  # torch is optional on the single-GPU path: the scores then come back as a host array
            torch = None
    if device and torch is not None:
        out = torch.empty((n, item.rows), dtype=torch.float32, device=torch.device("cuda", user.ctx.device))
        user.ctx.after_torch(out)            # (a cached block may still have work of torch's stream pending: the library's stream waits for it)
        check(lib.orx_score_all_items_device(*head, out.data_ptr()))
        return DeviceScores(user.ctx, out)
    out = np.empty((n, item.rows), np.float32)
    check(lib.orx_score_all_items(*head, out.ctypes.data))
    return out


TOPK_MAX_K = 1024


def _topk_k(k):
    k = int(k)
    if not 1 <= k <= TOPK_MAX_K:
        raise ValueError(f"k = {k} outside [1, {TOPK_MAX_K}]")
    return k


def _excl_lists(excl, n, items):
    """an exclusion mask as CSR item lists -> (ptr, items) or (None, None)"""
    if excl is None:
        return None, None
    if not isinstance(excl, SparseMask):
        excl = SparseMask.from_dense(excl)
    if excl.shape != (n, items):
        raise ValueError(f"exclusion mask of shape {excl.shape}, expected {(n, items)}")
    return excl.ptr, excl.items


def recommend_topk(kind, user, item, bias, uid, k, excl=None, w=None, device=False):
    """The k best items of each user -> (item ids int32 [n, k], scores float32 [n, k]), without the [n, item_rows] score
    matrix.  Scores are bit-identical to `score_all_items`; order: score descending, then item id ascending; items in
    `excl` (a SparseMask, or a dense bool mask [n, item_rows]) and NaN scores are skipped, and a row with fewer than k such
    items ends in item -1 / score -inf.  `device=True`: two torch tensors in HBM instead of host arrays."""
    lib = user.ctx._lib
    ptr, n, keep = _host_uid("recommend_topk", uid)
    k = _topk_k(k)
    kd = _kind_arg(kind)
    ep, ei = _excl_lists(excl, n, item.rows)
    head = (user.ctx._h, kd, *_scorer_head(user, item, bias, w), ptr, n,
            ep.ctypes.data if ep is not None else None, ei.ctypes.data if ei is not None else None, k)
    if device:
        import torch
        dv = torch.device("cuda", user.ctx.device)
        items_t = torch.empty((n, k), dtype=torch.int32, device=dv)
        scores_t = torch.empty((n, k), dtype=torch.float32, device=dv)
        user.ctx.after_torch(items_t, scores_t)
        check(lib.orx_recommend_topk(*head, _ffi.ORX_OUT_DEVICE, items_t.data_ptr(), scores_t.data_ptr()))
        return items_t, scores_t
    items_h = np.empty((n, k), np.int32)
    scores_h = np.empty((n, k), np.float32)
    check(lib.orx_recommend_topk(*head, 0, items_h.ctypes.data, scores_h.ctypes.data))
    return items_h, scores_h


def topk_rows(scores, k, excl=None, ctx=None):
    """The same selection over scores that exist already: a DeviceScores (read in HBM) or a host array [n, m]
    -> (item ids int32 [n, k], scores float32 [n, k]) on the host."""
    k = _topk_k(k)
    keep = None
    if isinstance(scores, DeviceScores) or _is_device_tensor(scores):
        t = scores.tensor if isinstance(scores, DeviceScores) else scores
        c = ctx or (scores.ctx if isinstance(scores, DeviceScores) else default_context())
        if t.dim() != 2:
            raise ValueError(f"topk_rows takes [n, m] scores, got shape {tuple(t.shape)}")
        keep = t.float().contiguous()
        if keep.data_ptr() != t.data_ptr():
            c.after_torch(keep)
        n, m = keep.shape
        head = (keep.data_ptr(), 1)
    else:
        keep = np.ascontiguousarray(scores, np.float32)
        if keep.ndim != 2:
            raise ValueError(f"topk_rows takes [n, m] scores, got shape {keep.shape}")
        c = ctx or default_context()
        n, m = keep.shape
        head = (keep.ctypes.data, 0)
    ep, ei = _excl_lists(excl, n, m)
    items_h = np.empty((n, k), np.int32)
    scores_h = np.empty((n, k), np.float32)
    check(c._lib.orx_topk_rows(c._h, *head, n, m, ep.ctypes.data if ep is not None else None,
                               ei.ctypes.data if ei is not None else None, k, items_h.ctypes.data, scores_h.ctypes.data))
    return items_h, scores_h


class _BorrowedTable(Table):
    """A table handle owned by another object (e.g. a DLRM model's parameter)."""

    def __init__(self, ctx, handle, owner):
        self.ctx, self._lib, self._h = ctx, ctx._lib, handle
        self.rows, self.dim = int(self._lib.orx_table_rows(handle)), int(self._lib.orx_table_dim(handle))
        self._keepalive = (owner, ctx)


class DLRMModel:
    """Device-side DLRM (recommenders/dlrm.py:6-100): combined embedding table,
    bottom / top MLPs, feature interaction, loss; `step` = forward + backward +
    optimizer apply of tf2_examples/dlrm_criteo.py:42-48."""

    def __init__(self, m_spa, ln_emb, ln_bot, ln_top, dense_dim, arch_interaction_itself=False, sigmoid_bot=False,
                 sigmoid_top=True, loss_func="mse", loss_threshold=0.0, reference_compat=True, seed=0, ctx=None,
                 fp16_mlp=False, no_emb=False):
        self.ctx = ctx or default_context()
        lib = self._lib = self.ctx._lib
        self.m_spa, self.ln_emb, self.ln_bot, self.ln_top = int(m_spa), [int(x) for x in ln_emb], list(ln_bot), list(ln_top)
        self.dense_dim = int(dense_dim)
        self.loss_func = loss_func
        flags = ((_ffi.ORX_DLRM_INTERACT_ITSELF if arch_interaction_itself else 0)
                 | (_ffi.ORX_DLRM_SIGMOID_BOT if sigmoid_bot else 0) | (_ffi.ORX_DLRM_SIGMOID_TOP if sigmoid_top else 0)
                 | (_ffi.ORX_DLRM_LOSS_BCE if loss_func == "bce" else 0)
                 | (_ffi.ORX_DLRM_REFERENCE_COMPAT if reference_compat else 0)
                 | (_ffi.ORX_DLRM_FP16_MLP if fp16_mlp else 0) | (_ffi.ORX_DLRM_NO_EMB if no_emb else 0))
        if loss_func not in ("mse", "bce"):
            raise ValueError("loss_func=%s is not supported" % loss_func)          # dlrm.py:56-61
        emb = (ctypes.c_int64 * len(self.ln_emb))(*self.ln_emb)
        bot = (ctypes.c_int32 * len(ln_bot))(*ln_bot)
        top = (ctypes.c_int32 * len(ln_top))(*ln_top)
        h = c_void_p()
        check(lib.orx_dlrm_create(self.ctx._h, self.m_spa, len(self.ln_emb), ctypes.cast(emb, c_void_p),
                                  len(ln_bot), ctypes.cast(bot, c_void_p), len(ln_top), ctypes.cast(top, c_void_p),
                                  self.dense_dim, flags, float(loss_threshold), int(seed), byref(h)))
        self._h = h
        self._fin = weakref.finalize(self, lib.orx_dlrm_destroy, h)
        self.offsets = np.concatenate([[0], np.cumsum(self.ln_emb)[:-1]]).astype(np.int64)

    def param(self, kind, layer=0):
        k = {"emb": 0, "bot_w": 1, "bot_b": 2, "top_w": 3, "top_b": 4}[kind]
        h = c_void_p()
        check(self._lib.orx_dlrm_param(self._h, k, int(layer), byref(h)))
        return _BorrowedTable(self.ctx, h, self)

    def emb_table(self, f):
        """numpy view helper: rows of embedding table f inside the combined table"""
        return int(self.offsets[f]), self.ln_emb[f]

    @staticmethod
    def _host(x, dtype):
        if hasattr(x, "numpy") and not isinstance(x, np.ndarray):
            x = x.numpy()
        return np.ascontiguousarray(x, dtype=dtype)

    def step_device(self, opt, dense_ptr, sparse_ptr, label_ptr, K, B, want_loss=False):
        """K steps on batches that already sit in HBM (device pointers, layout as `step`)."""
        loss = np.empty(K, np.float32) if want_loss else None
        check(self._lib.orx_dlrm_step(self._h, opt._h, dense_ptr, sparse_ptr, label_ptr, int(K), int(B), _ffi.ORX_IDS_DEVICE,
                                      loss.ctypes.data if want_loss else None))
        opt._tables.append(self)
        return loss

    def step(self, opt, dense, sparse, label, K=1, want_loss=True):
        d, s, y = self._host(dense, np.float32), self._host(sparse, np.int32), self._host(label, np.float32)
        B = y.size // K
        assert d.size == K * B * self.dense_dim and s.size == K * B * len(self.ln_emb)
        loss = np.empty(K, np.float32) if want_loss else None
        check(self._lib.orx_dlrm_step(self._h, opt._h, d.ctypes.data, s.ctypes.data, y.ctypes.data, K, B, 0,
                                      loss.ctypes.data if want_loss else None))
        opt._tables.append(self)
        return loss

    # ---- hybrid-parallel building blocks (device pointers; openrec_amd/sharded_dlrm.py) ----
    def grads(self, dense_ptr, emb_rows_ptr, label_ptr, B, global_B, emb_grads_ptr, loss_accum_ptr):
        check(self._lib.orx_dlrm_grads(self._h, dense_ptr, emb_rows_ptr, label_ptr, int(B), int(global_B),
                                       emb_grads_ptr, loss_accum_ptr))

    def dense_count(self):
        n = ctypes.c_int64()
        check(self._lib.orx_dlrm_dense_count(self._h, byref(n)))
        return int(n.value)

    def dense_pack(self, flat_ptr):
        check(self._lib.orx_dlrm_dense_pack(self._h, flat_ptr))

    def dense_apply(self, opt, flat_ptr):
        check(self._lib.orx_dlrm_dense_apply(self._h, opt._h, flat_ptr))
        opt._tables.append(self)

    def inference(self, dense, sparse):
        d, s = self._host(dense, np.float32), self._host(sparse, np.int32)
        B = d.size // self.dense_dim
        out = np.empty(B, np.float32)
        check(self._lib.orx_dlrm_inference(self._h, d.ctypes.data, s.ctypes.data, B, 0, out.ctypes.data))
        return out


def rank_metrics(pos_mask, excl_mask, at, pred=None, kind=None, user=None, item=None, bias=None, w=None, uid=None, ctx=None):
    """AUC / NDCG@at / Recall@at per user (openrec/tf2/metrics/ranking_metrics.py).  Either `pred`
    (host scores [n, items]) or the tables + user ids (scores computed on the device)."""
    pos = np.ascontiguousarray(pos_mask, np.uint8)
    excl = np.ascontiguousarray(excl_mask, np.uint8)
    n, items = pos.shape
    atv, auc, ndcg, rec, result = _metric_outputs(n, at)
    c = ctx or (user.ctx if user is not None else default_context())
    if pred is not None:
        pr = np.ascontiguousarray(pred, np.float32)
        assert pr.shape == (n, items)
        check(c._lib.orx_rank_metrics(c._h, 0, None, None, None, None, None, pr.ctypes.data, pos.ctypes.data, excl.ctypes.data,
                                      n, items, atv.ctypes.data, atv.size, auc.ctypes.data, ndcg.ctypes.data, rec.ctypes.data))
    else:
        ptr, nn, dev, keep = _ids_arg(uid)
        assert nn == n and not dev
        check(c._lib.orx_rank_metrics(c._h, _kind_arg(kind), *_scorer_head(user, item, bias, w), ptr, None,
                                      pos.ctypes.data, excl.ctypes.data, n, items, atv.ctypes.data, atv.size,
                                      auc.ctypes.data, ndcg.ctypes.data, rec.ctypes.data))
    return result


def rank_metrics_csr(pos, excl, at, pred=None, kind=None, user=None, item=None, bias=None, w=None, uid=None, ctx=None):
    """`rank_metrics` with the masks as SparseMask (item lists): nothing of size n x items crosses PCIe when the scores are
    on the device (`pred` a DeviceScores, or None with the tables + user ids)."""
    assert isinstance(pos, SparseMask) and isinstance(excl, SparseMask) and pos.shape == excl.shape
    n, items = pos.shape
    atv, auc, ndcg, rec, result = _metric_outputs(n, at)
    c = ctx or (user.ctx if user is not None else (pred.ctx if isinstance(pred, DeviceScores) else default_context()))
    tail = (n, items, pos.ptr.ctypes.data, pos.items.ctypes.data, excl.ptr.ctypes.data, excl.items.ctypes.data,
            atv.ctypes.data, atv.size, auc.ctypes.data, ndcg.ctypes.data, rec.ctypes.data)
    if pred is not None:
        if isinstance(pred, DeviceScores):
            assert pred.shape == (n, items)
            head = (pred.tensor.data_ptr(), 1)
        else:
            pr = np.ascontiguousarray(pred, np.float32)
            assert pr.shape == (n, items)
            head = (pr.ctypes.data, 0)
        check(c._lib.orx_rank_metrics_csr(c._h, 0, None, None, None, None, None, *head, *tail))
    else:
        ptr, nn, dev, keep = _ids_arg(uid)
        assert nn == n and not dev
        check(c._lib.orx_rank_metrics_csr(c._h, _kind_arg(kind), *_scorer_head(user, item, bias, w), ptr, None, 0, *tail))
    return result


def rank_metrics_matrixfree_scratch(n, items, dim, kind, max_pos, max_excl, scratch_bytes=0, ctx=None):
    """(bytes, users_per_batch): the device scratch `rank_metrics_matrixfree` would make for such a call, and the users it
    would take per batch.  Host only."""
    lib = ctx._lib if ctx is not None else _ffi.load()
    b, u = ctypes.c_int64(), ctypes.c_int64()
    check(lib.orx_rank_metrics_matrixfree_scratch(int(n), int(items), int(dim), _kind_arg(kind), int(max_pos), int(max_excl), int(scratch_bytes),
                                                  byref(b), byref(u)))
    return int(b.value), int(u.value)


def rank_metrics_matrixfree_check(pos, excl):
    """The list checks `rank_metrics_matrixfree` makes before any device work -> (longest positive list, longest exclusion
    list).  ValueError for a row that is not strictly ascending, IndexError for an id outside the table.  Host only."""
    assert isinstance(pos, SparseMask) and isinstance(excl, SparseMask) and pos.shape == excl.shape
    mp, me = ctypes.c_int64(), ctypes.c_int64()
    check(_ffi.load().orx_rank_metrics_matrixfree_check(pos.shape[0], pos.shape[1], pos.ptr.ctypes.data, pos.items.ctypes.data,
                                                        excl.ptr.ctypes.data, excl.items.ctypes.data, byref(mp), byref(me)))
    return int(mp.value), int(me.value)


def rank_metrics_matrixfree(pos, excl, at, kind, user, item, bias, uid, w=None, scratch_bytes=0):
    """`rank_metrics_csr(pos, excl, at, kind=..., ...)` without the [n, item_rows] score matrix or the two bitmaps: the same
    numbers bit for bit, from device scratch that stays within `scratch_bytes` (0: 512 MB) however many users and items there
    are.  `pos` / `excl`: SparseMask whose rows are strictly ascending (what from_lists / from_dense make)."""
    assert isinstance(pos, SparseMask) and isinstance(excl, SparseMask) and pos.shape == excl.shape
    n, items = pos.shape
    if items != item.rows:
        raise ValueError(f"masks over {items} items, the item table has {item.rows} rows")
    atv, auc, ndcg, rec, result = _metric_outputs(n, at)
    ptr, _, keep = _host_uid("rank_metrics_matrixfree", uid, n)
    c = user.ctx
    check(c._lib.orx_rank_metrics_matrixfree(c._h, _kind_arg(kind), *_scorer_head(user, item, bias, w), ptr, n,
                                             pos.ptr.ctypes.data, pos.items.ctypes.data, excl.ptr.ctypes.data, excl.items.ctypes.data,
                                             atv.ctypes.data, atv.size, int(scratch_bytes), auc.ctypes.data, ndcg.ctypes.data,
                                             rec.ctypes.data))
    return result


class CandidateLists(_ItemLists):
    """One list of item ids per user, kept in the GIVEN order and with its repeats (a re-ranker's input is ordered by the
    retrieval stage): `ptr` int64 [n + 1] from 0, `items` int32.  `SparseMask` is the sorted, distinct form."""

    @classmethod
    def from_lists(cls, lists, n_items):
        rows = [np.asarray(r, np.int64).reshape(-1) for r in lists]
        ptr = np.zeros(len(rows) + 1, np.int64); np.cumsum([r.size for r in rows], out=ptr[1:])
        items = np.concatenate(rows) if rows else np.zeros(0, np.int64)
        if items.size and (items.min() < 0 or items.max() >= n_items):
            raise IndexError(f"item id outside [0, {n_items})")
        return cls(ptr, items.astype(np.int32), n_items)


def as_candidate_lists(cand, n_items):
    """a SparseMask, a CandidateLists or a list of per-user id arrays (order kept) -> an object with ptr / items / shape"""
    if isinstance(cand, (SparseMask, CandidateLists)):
        return cand
    return CandidateLists.from_lists(cand, n_items)


def score_candidates(kind, user, item, bias, uid, cand, w=None, device=False):
    """The scores of each user's own candidates -> flat float32 [len(cand.items)] aligned with `cand.items` (with
    `device=True` a torch tensor in HBM).  `cand`: a SparseMask, a CandidateLists, or a list of per-user id arrays kept in the
    given order (repeats allowed).  Every score equals `score_all_items(...)[q, item]` bit for bit; only the listed items are
    scored, so neither work nor memory grows with users x items."""
    lib = user.ctx._lib
    ptr, n, keep = _host_uid("score_candidates", uid)
    cand = as_candidate_lists(cand, item.rows)
    if cand.shape != (n, item.rows):
        raise ValueError(f"candidate lists of shape {cand.shape}, expected {(n, item.rows)}")
    total = int(cand.ptr[-1])
    head = (user.ctx._h, _kind_arg(kind), *_scorer_head(user, item, bias, w), ptr, n,
            cand.ptr.ctypes.data, cand.items.ctypes.data)
    if device:
        import torch
        out_t = torch.empty((total,), dtype=torch.float32, device=torch.device("cuda", user.ctx.device))
        user.ctx.after_torch(out_t)
        check(lib.orx_score_candidates(*head, _ffi.ORX_OUT_DEVICE, out_t.data_ptr()))
        return out_t
    out = np.empty(total, np.float32)
    check(lib.orx_score_candidates(*head, 0, out.ctypes.data))
    return out


def rank_metrics_candidates_check(pos, cand):
    """The list checks `rank_metrics_candidates` makes before any device work -> (longest positive list, longest candidate
    list).  ValueError naming user and list for a row that is not strictly ascending, IndexError for an id outside the table.
    Host only."""
    assert pos.shape == cand.shape
    mp, mc = ctypes.c_int64(), ctypes.c_int64()
    check(_ffi.load().orx_rank_metrics_candidates_check(pos.shape[0], pos.shape[1], pos.ptr.ctypes.data, pos.items.ctypes.data,
                                                        cand.ptr.ctypes.data, cand.items.ctypes.data, byref(mp), byref(mc)))
    return int(mp.value), int(mc.value)


def rank_metrics_candidates(pos, cand, at, kind, user, item, bias, uid, w=None, scratch_bytes=0):
    """AUC / NDCG / Recall of each user over the universe `cand[q]` (sampled or explicit negatives plus the positives):
    bit for bit `rank_metrics_csr(pos, ~cand, at, kind=..., ...)`, but only the listed items are scored and nothing of size
    users x items exists anywhere.  `pos` / `cand`: SparseMask whose rows are strictly ascending; device scratch stays within
    `scratch_bytes` (0: 512 MB)."""
    assert isinstance(pos, SparseMask) and isinstance(cand, (SparseMask, CandidateLists)) and pos.shape == cand.shape
    n, items = pos.shape
    if items != item.rows:
        raise ValueError(f"masks over {items} items, the item table has {item.rows} rows")
    atv, auc, ndcg, rec, result = _metric_outputs(n, at)
    ptr, _, keep = _host_uid("rank_metrics_candidates", uid, n)
    c = user.ctx
    check(c._lib.orx_rank_metrics_candidates(c._h, _kind_arg(kind), *_scorer_head(user, item, bias, w), ptr, n,
                                             pos.ptr.ctypes.data, pos.items.ctypes.data, cand.ptr.ctypes.data, cand.items.ctypes.data,
                                             atv.ctypes.data, atv.size, int(scratch_bytes), auc.ctypes.data, ndcg.ctypes.data,
                                             rec.ctypes.data))
    return result


CKPT_PIECE_BYTES = 256 << 20          # tables and slots move through the host in pieces of at most this many bytes


def _stream_rows(read, rows, dim, dst):
    """rows [0, rows) through `read(row0, n) -> [n, dim]` into the (memory-mapped) array `dst`, CKPT_PIECE_BYTES at a time"""
    step = max(1, CKPT_PIECE_BYTES // max(1, 4 * dim))
    for r0 in range(0, rows, step):
        n = min(step, rows - r0)
        dst[r0:r0 + n] = read(r0, n)


def save_checkpoint(path, tables, opt=None, shard=None):
    """Tables (and the optimizer's slots for them) -> a checkpoint.  The tf2 reference has no checkpointing (`save_interval` is
    unused, tf2_examples/bpr_citeulike.py:16); tf1 used tf.train.Saver (tf1/recommenders/recommender.py:430-473).
    `tables`: {name: Table}.

    `path` ending in ".npz": ONE file, every tensor whole in host memory on the way (small models, the round-1 format).
    Otherwise `path` is a DIRECTORY: one .npy per tensor -- `table.<name>.npy`, `slot0.<name>.npy`, `slot1.<name>.npy` -- written
    through a memory map in row ranges of at most CKPT_PIECE_BYTES (a 10 M x 128 table never sits in host memory whole), and
    `manifest.json` (shapes, optimizer kind and step counter).  `shard=(rank, world)`: this rank's files get the suffix
    `.rank<r>of<w>` and the manifest records the sharding (row r of the global table = local row r // world of rank r % world,
    SURVEY.md 8(e)): every rank of a row-sharded job saves its own shard into the same directory."""
    import json
    if str(path).endswith(".npz"):
        out = {}
        for name, t in tables.items():
            out["table/" + name] = t.read()
            if opt is not None and opt.kind in ("adagrad", "adam", "momentum"):
                out["slot0/" + name] = opt.slot(t, 0)
                if opt.kind == "adam":
                    out["slot1/" + name] = opt.slot(t, 1)
        if opt is not None:
            out["opt/kind"] = np.array(opt.kind)
            out["opt/step"] = np.array(opt.step, np.int64)          # Adam's bias correction resumes where it stopped
            if opt.kind == "momentum":
                out["opt/momentum"] = np.array(opt.params[:2], np.float32)      # (momentum, nesterov)
        np.savez(path, **out)
        return
    os.makedirs(path, exist_ok=True)
    suffix = "" if shard is None else ".rank%dof%d" % (int(shard[0]), int(shard[1]))
    man = dict(format="openrec_amd-ckpt-1", tensors={}, shard=None if shard is None else dict(rank=int(shard[0]), world=int(shard[1])))
    nslots = 0 if opt is None else Optimizer.NSLOTS[opt.kind]
    for name, t in tables.items():
        if hasattr(t, "_sync_pending"):
            t._sync_pending()
        man["tensors"][name] = dict(rows=t.rows, dim=t.dim, slots=nslots)
        mm = np.lib.format.open_memmap(os.path.join(path, f"table.{name}{suffix}.npy"), mode="w+", dtype=np.float32, shape=(t.rows, t.dim))
        _stream_rows(t.read, t.rows, t.dim, mm)
        mm.flush(); del mm
        for k in range(nslots):
            mm = np.lib.format.open_memmap(os.path.join(path, f"slot{k}.{name}{suffix}.npy"), mode="w+", dtype=np.float32, shape=(t.rows, t.dim))
            _stream_rows(lambda r0, n, k=k: opt.slot_rows(t, k, r0, n), t.rows, t.dim, mm)
            mm.flush(); del mm
    if opt is not None:
        man["opt"] = dict(kind=opt.kind, step=int(opt.step))
        if opt.kind == "momentum":
            man["opt"].update(momentum=opt.params[0], nesterov=bool(opt.params[1]))
    with open(os.path.join(path, f"manifest{suffix}.json"), "w") as f:
        json.dump(man, f, indent=1)


def _check_momentum(path, saved, opt):
    """a velocity only continues under the momentum and the nesterov flag it was accumulated with"""
    want = (float(np.float32(opt.params[0])), opt.params[1])
    if (float(np.float32(saved[0])), saved[1]) != want:
        raise ValueError(f"{path}: saved with momentum={saved[0]:g}, nesterov={bool(saved[1])}; "
                         f"the optimizer has momentum={opt.params[0]:g}, nesterov={bool(opt.params[1])}")


def load_checkpoint(path, tables, opt=None, shard=None):
    """the inverse of save_checkpoint (same `path` / `shard` conventions); shapes and the optimizer kind are checked"""
    import json
    if str(path).endswith(".npz"):
        z = np.load(path)
        saved = str(z["opt/kind"]) if "opt/kind" in z else None
        if opt is not None and saved is not None and saved != opt.kind and "momentum" in (saved, opt.kind):
            raise ValueError(f"{path}: saved with a {saved} optimizer, loading into {opt.kind}")     # (a velocity is no other slot)
        if opt is not None and opt.kind == "momentum" and "opt/momentum" in z:
            _check_momentum(path, tuple(float(v) for v in z["opt/momentum"]), opt)
        for name, t in tables.items():
            t.write(z["table/" + name])
            if opt is not None and ("slot0/" + name) in z:
                opt.set_slot(t, z["slot0/" + name], 0)
                if ("slot1/" + name) in z:
                    opt.set_slot(t, z["slot1/" + name], 1)
        if opt is not None and "opt/step" in z:
            opt.step = int(z["opt/step"])
        return
    suffix = "" if shard is None else ".rank%dof%d" % (int(shard[0]), int(shard[1]))
    with open(os.path.join(path, f"manifest{suffix}.json")) as f:
        man = json.load(f)
    if man.get("format") != "openrec_amd-ckpt-1":
        raise ValueError(f"{path}: not an openrec_amd checkpoint directory")
    want_shard = None if shard is None else dict(rank=int(shard[0]), world=int(shard[1]))
    if man.get("shard") != want_shard:
        raise ValueError(f"{path}: saved with shard={man.get('shard')}, asked for {want_shard}")
    if opt is not None and "opt" in man and man["opt"]["kind"] != opt.kind:
        raise ValueError(f"{path}: saved with a {man['opt']['kind']} optimizer, loading into {opt.kind}")
    if opt is not None and opt.kind == "momentum" and "momentum" in man.get("opt", {}):
        _check_momentum(path, (float(man["opt"]["momentum"]), 1.0 if man["opt"]["nesterov"] else 0.0), opt)
    for name, t in tables.items():
        info = man["tensors"].get(name)
        if info is None:
            raise KeyError(f"{path}: no tensor named {name!r}")
        if (info["rows"], info["dim"]) != (t.rows, t.dim):
            raise ValueError(f"{path}: {name} is [{info['rows']}, {info['dim']}], the table [{t.rows}, {t.dim}]")
        step = max(1, CKPT_PIECE_BYTES // max(1, 4 * t.dim))
        mm = np.load(os.path.join(path, f"table.{name}{suffix}.npy"), mmap_mode="r")
        for r0 in range(0, t.rows, step):
            t.write(np.ascontiguousarray(mm[r0:r0 + step]), r0)
        del mm
        if opt is not None:
            for k in range(min(info["slots"], Optimizer.NSLOTS[opt.kind])):
                mm = np.load(os.path.join(path, f"slot{k}.{name}{suffix}.npy"), mmap_mode="r")
                for r0 in range(0, t.rows, step):
                    opt.set_slot_rows(t, np.ascontiguousarray(mm[r0:r0 + step]), k, r0)
                del mm
    if opt is not None and "opt" in man:
        opt.step = int(man["opt"]["step"])


def alias_build(weights):
    """The Walker / Vose alias table of `weights` (floats >= 0, not all 0) -> (thr uint32[n], alias int32[n]): with a uniform
    32-bit t, column j yields j if t < thr[j] and alias[j] otherwise; a uniform column then draws item i in proportion to
    weights[i].  An item of weight 0 is never an outcome.  ValueError for an empty array, a NaN, infinite or negative weight or
    weights that are all 0.  Host only: no context, no device."""
    w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    thr, alias = np.empty(w.size, np.uint32), np.empty(w.size, np.int32)
    check(_ffi.load().orx_alias_build(w.ctypes.data, w.size, thr.ctypes.data, alias.ctypes.data))
    return thr, alias


WARP_KINDS = ("log", "log1p", "harmonic")


def warp_weights(total_items, max_trials, kind="log", normalize=False):
    """The weight table of `DeviceSampler.pairwise_warp` -> float32[max_trials]: entry t - 1 is the rank loss of a triplet whose
    first violating candidate was the t-th drawn, a function of WARP's rank estimate r_t = floor((total_items - 1) / t):
    "log": log(max(1, r_t)) (LightFM), "log1p": log(r_t + 1) (CML), "harmonic": sum_{i <= r_t} 1 / i (WSABIE).  Computed in
    float64 and cast once; normalize=True divides by the entry of t = 1 first.  ValueError for total_items < 2, max_trials outside
    [1, 256] or an unknown kind.  Host only: no context, no device."""
    total_items, max_trials = int(total_items), int(max_trials)
    if total_items < 2:
        raise ValueError("warp_weights: total_items must be at least 2, got %d" % total_items)
    if not 1 <= max_trials <= 256:
        raise ValueError("warp_weights: max_trials must be in [1, 256], got %d" % max_trials)
    if kind not in WARP_KINDS:
        raise ValueError("warp_weights: kind must be one of %s, got %r" % (", ".join(WARP_KINDS), kind))
    r = (total_items - 1) // np.arange(1, max_trials + 1, dtype=np.int64)
    if kind == "log":
        w = np.log(np.maximum(1, r).astype(np.float64))
    elif kind == "log1p":
        w = np.log((r + 1).astype(np.float64))
    else:
        h = np.concatenate([[0.0], np.cumsum(1.0 / np.arange(1, int(r[0]) + 1, dtype=np.float64))])
        w = h[r]
    if normalize:
        w = w / w[0]
    return w.astype(np.float32)


# The sampler's argument helpers (plain functions with positional arguments: a producer call is a few microseconds of host time)
def _sampler_out(arg, x, n, what, optional=False):
    """the pointer of the DEVICE output buffer `x` of at least n elements -- int32 for arg = _ids_arg, float32 for _label_arg --;
    None where `optional` and not given"""
    if x is None and optional:
        return None
    ptr, size, on_device, _ = arg(x)
    assert on_device and size >= n, "%s: the sampler writes a device buffer of %d" % (what, n)
    return ptr


def _sampler_model(model):
    return int(model if isinstance(model, int) else {"bpr": _ffi.ORX_BPR, "ucml": _ffi.ORX_UCML}[model])


def _seed_arg(seed):
    return int(seed) & (2 ** 64 - 1)


def _scorer_handles(U, V, b):
    for t in (U, V, b):
        if t is not None:
            t._sync_pending()
    return U._h, V._h, _bias_h(b)


class DeviceSampler:
    """On-device pairwise sampler over an interaction set (see kernels_sampler.hip).  `raw_data`: the
    structured array the reference's Dataset takes ('user_id', 'item_id')."""

    def __init__(self, raw_data, total_users, total_items, ctx=None):
        self.ctx = ctx or default_context()
        lib = self._lib = self.ctx._lib
        u = np.ascontiguousarray(raw_data["user_id"], np.int32)
        i = np.ascontiguousarray(raw_data["item_id"], np.int32)
        key = np.unique(u.astype(np.int64) * int(total_items) + i)            # sorted by (user, item), distinct
        cu, ci = (key // int(total_items)).astype(np.int64), (key % int(total_items)).astype(np.int32)
        ptr = np.zeros(int(total_users) + 1, np.int64)
        np.add.at(ptr, cu + 1, 1)
        ptr = np.ascontiguousarray(np.cumsum(ptr), np.int64)
        ci = np.ascontiguousarray(ci)
        h = c_void_p()
        check(lib.orx_sampler_create(self.ctx._h, u.ctypes.data, i.ctypes.data, u.size, ptr.ctypes.data, ci.ctypes.data,
                                     int(total_users), int(total_items), byref(h)))
        self._h, self.n_records = h, int(u.size)
        self._fin = weakref.finalize(self, lib.orx_sampler_destroy, h)
        self.total_items = int(total_items)
        self._item_users = np.bincount(ci, minlength=int(total_items)).astype(np.float64)     # distinct users per item
        self._has_proposal = False
        self._warp_tables = {}

    def set_proposal(self, weights=None, *, popularity=None):
        """Draw the negatives of `pairwise` and the candidates of `pairwise_hard` from a weighted proposal over the items
        instead of uniformly: an item comes up in proportion to its weight (then, as always, re-drawn while it is a positive of
        the user), an item of weight 0 never.  `weights`: a float array of total_items, >= 0 and not all 0.  `popularity=alpha`
        builds the weights from the sampler's own interactions: (the number of distinct users of the item) ** alpha, 0.75 being
        the word2vec value.  An item nobody interacted with has weight 0 if alpha > 0 and weight 1 (= 0 ** 0, like every other
        item) if alpha == 0, so popularity=0 is the uniform proposal over the whole catalogue.  Neither argument (or
        weights=None): uniform negatives again, bit for bit the stream of a sampler that never had a proposal.  Giving both is
        a ValueError, and so are bad weights -- the proposal in force then stays in force.  The call may synchronise the
        context's stream: draws enqueued before it use the old proposal.  The pointwise producers raise while one is set."""
        if weights is not None and popularity is not None:
            raise ValueError("set_proposal: give weights or popularity=alpha, not both")
        if popularity is not None:
            alpha = float(popularity)
            if not np.isfinite(alpha) or alpha < 0:
                raise ValueError("set_proposal: popularity=alpha needs a finite alpha >= 0, got %r" % (popularity,))
            weights = np.ones(self.total_items) if alpha == 0 else self._item_users ** alpha
        if weights is None:
            check(self._lib.orx_sampler_set_proposal(self._h, None))
            self._has_proposal = False
            return
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if w.size != self.total_items:
            raise ValueError("set_proposal: %d weights for %d items" % (w.size, self.total_items))
        check(self._lib.orx_sampler_set_proposal(self._h, w.ctypes.data))
        self._has_proposal = True

    def proposal(self):
        """(thr uint32[total_items], alias int32[total_items]) read back from the device -- `alias_build` of the weights in
        force -- or None when no proposal is set"""
        if not self._has_proposal:
            return None
        thr, alias = np.empty(self.total_items, np.uint32), np.empty(self.total_items, np.int32)
        check(self._lib.orx_sampler_proposal_read(self._h, thr.ctypes.data, alias.ctypes.data))
        return thr, alias

    def pairwise(self, seed, first, n, uid, pid, nid):
        """Fill the DEVICE int32 buffers uid / pid / nid (torch tensors or DevicePtr) with samples
        [first, first + n) of stream `seed`.  Negatives: uniform over the user's non-positives, or from `set_proposal`'s."""
        check(self._lib.orx_sampler_pairwise(self._h, _seed_arg(seed), int(first), int(n), _sampler_out(_ids_arg, uid, n, "uid"),
                                             _sampler_out(_ids_arg, pid, n, "pid"), _sampler_out(_ids_arg, nid, n, "nid")))

    def set_record_weights(self, weights=None):
        """One weight per interaction record, in the order of `raw_data` (float32; not validated), kept on the device for
        `pairwise_weights`; None drops them.  The call may synchronise the context's stream."""
        if weights is None:
            check(self._lib.orx_sampler_set_record_weights(self._h, None))
            return
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        if w.size != self.n_records:
            raise ValueError("set_record_weights: %d weights for %d records" % (w.size, self.n_records))
        check(self._lib.orx_sampler_set_record_weights(self._h, w.ctypes.data))

    def pairwise_weights(self, seed, first, n, out):
        """Fill the DEVICE float32 buffer `out` with the record weights of samples [first, first + n) of stream `seed`: out[i]
        is the weight of the (user, positive) record that `pairwise` / `pairwise_hard` write at i for the same (seed, first),
        with or without a proposal -- ready to be `pairwise_step`'s weights.  Raises OrxError (ORX_ERR_STATE) while no record
        weights are set."""
        check(self._lib.orx_sampler_pairwise_weights(self._h, _seed_arg(seed), int(first), int(n), _sampler_out(_label_arg, out, n, "out")))

    def pairwise_hard(self, seed, first, n, uid, pid, nid, model, U, V, b=None, candidates=8,
                      cand_out=None, cand_score_out=None):
        """Dynamic negative sampling: uid / pid as `pairwise(seed, first, n)` writes them, nid the hardest of `candidates`
        uniform non-positive items of the user -- the one `model` ("bpr": U[u].V[c] + b[c], "ucml": -|U[u] - V[c]|^2 + b[c];
        b=None: no bias) scores highest on the tables as they stand.  Candidate c depends on (seed, sample, c) only and
        candidate 0 is `pairwise`'s negative, so candidates=1 is `pairwise` bit for bit.  Equal scores: the smallest c; NaN
        never wins.  cand_out (int32) / cand_score_out (float32): optional DEVICE buffers [n * candidates] that receive every
        candidate and its score.  All buffers are device buffers; the call runs on the context's stream without a host
        synchronisation, so its output can feed `pairwise_step` directly.  1 <= candidates <= 64.  With `set_proposal` the
        candidates come from the proposal instead of uniformly; everything else stays as described."""
        M = int(candidates)
        outs = (_sampler_out(_ids_arg, uid, n, "uid"), _sampler_out(_ids_arg, pid, n, "pid"), _sampler_out(_ids_arg, nid, n, "nid"),
                _sampler_out(_ids_arg, cand_out, n * M, "cand_out", True), _sampler_out(_label_arg, cand_score_out, n * M, "cand_score_out", True))
        check(self._lib.orx_sampler_pairwise_hard(self._h, _sampler_model(model), *_scorer_handles(U, V, b), _seed_arg(seed),
                                                  int(first), int(n), M, *outs))

    def pairwise_multi(self, seed, first, n, uid, pid, nid, negatives=16):
        """The negatives of `multineg_step`: uid / pid as `pairwise(seed, first, n)` writes them, and nid -- a DEVICE int32
        buffer [n, negatives] -- the first `negatives` candidates of `pairwise_hard` for every sample, bit for bit (candidate 0
        is `pairwise`'s negative; from the proposal when `set_proposal` is in force).  Only the draws: no table is read.
        1 <= negatives <= 64.  Runs on the context's stream without a host synchronisation."""
        N = int(negatives)
        if not 1 <= N <= 64:
            raise ValueError(f"pairwise_multi: negatives = {N}; must be in [1, 64]")
        check(self._lib.orx_sampler_pairwise_multi(self._h, _seed_arg(seed), int(first), int(n), N, _sampler_out(_ids_arg, uid, n, "uid"),
                                                   _sampler_out(_ids_arg, pid, n, "pid"), _sampler_out(_ids_arg, nid, n * N, "nid")))

    def pairwise_warp(self, seed, first, n, uid, pid, nid, weight, model, U, V, b=None, max_trials=10, margin=1.0,
                      rank_weight="log", trials_out=None, pos_score_out=None, cand_score_out=None):
        """WARP negative sampling: uid / pid as `pairwise(seed, first, n)` writes them; the candidates of `pairwise_hard`
        (candidate 0 is `pairwise`'s negative; from the proposal when `set_proposal` is in force) are taken one after another
        until one violates the margin against the positive under `model` on the tables as they stand ("bpr": U[u].V[j] + b[j],
        "ucml": -|U[u] - V[j]|^2 + b[j]; b=None: no bias).  Candidate c violates iff (s_c + margin) > s_p in fp32 -- one rounded
        add, then a compare; a NaN score never violates; margin may be +-inf, a NaN margin is a ValueError.  With t = 1 + the
        first violating candidate, or 0 when none of the `max_trials` (1 .. 256) violates:
            nid[i] = candidate t - 1 (candidate 0 when t = 0)        weight[i] = table[t - 1] (exactly +0.0 when t = 0)
        where `rank_weight` gives the table: a kind of `warp_weights(total_items, max_trials, kind)` or an array of max_trials
        floats.  `weight` is ready to be `pairwise_step(..., weights=weight)`: a weight of 0 leaves a triplet only its l2 part.
        trials_out (int32 [n]): t.  pos_score_out (float32 [n]): s_p.  cand_score_out (float32 [n * max_trials]): s_c for every
        c < t (every c < max_trials when t = 0); the entries beyond are unspecified.  A sample's outputs depend on (seed, first +
        i), the tables, the margin and the table only, never on n, first or the launch; a repeated call gives the same bits; for
        T1 < T2 a sample that found its violator within T1 keeps t and nid at T2.  The rank estimate floor((items - 1) / t) is
        WARP's for UNIFORM candidates; with a proposal set it estimates the rank under the proposal, not the uniform one.
        All buffers are device buffers; the call runs on the context's stream without a host synchronisation while the table
        stays the same (a changed table is uploaded and may synchronise the stream), so its output feeds `pairwise_step`."""
        T = int(max_trials)
        if not 1 <= T <= 256:
            raise ValueError("pairwise_warp: max_trials must be in [1, 256], got %d" % T)
        if isinstance(rank_weight, str):
            key = (rank_weight, T)
            if self._warp_tables.get("key") != key:
                self._warp_tables = {"key": key, "table": warp_weights(self.total_items, T, rank_weight)}
            table = self._warp_tables["table"]
        else:
            table = np.ascontiguousarray(rank_weight, dtype=np.float32).reshape(-1)
            if table.size != T:
                raise ValueError("pairwise_warp: rank_weight has %d entries, max_trials is %d" % (table.size, T))
        outs = (_sampler_out(_ids_arg, uid, n, "uid"), _sampler_out(_ids_arg, pid, n, "pid"), _sampler_out(_ids_arg, nid, n, "nid"),
                _sampler_out(_label_arg, weight, n, "weight"), _sampler_out(_ids_arg, trials_out, n, "trials_out", True),
                _sampler_out(_label_arg, pos_score_out, n, "pos_score_out", True), _sampler_out(_label_arg, cand_score_out, n * T, "cand_score_out", True))
        check(self._lib.orx_sampler_pairwise_warp(self._h, _sampler_model(model), *_scorer_handles(U, V, b), _seed_arg(seed),
                                                  int(first), int(n), T, float(margin), table.ctypes.data, *outs))

    def _pointwise(self, fn, seed, first, n, pos_ratio, uid, iid, label):
        check(fn(self._h, _seed_arg(seed), int(first), int(n), float(pos_ratio), _sampler_out(_ids_arg, uid, n, "uid"),
                 _sampler_out(_ids_arg, iid, n, "iid"), _sampler_out(_label_arg, label, n, "label")))

    def stratified_pointwise(self, seed, first, n, pos_ratio, uid, iid, label):
        """(user, item, label) samples [first, first + n) of `Dataset.stratified_pointwise` into DEVICE buffers; the stream
        is sequential (first = 0, then each call continues where the previous one stopped)."""
        self._pointwise(self._lib.orx_sampler_stratified, seed, first, n, pos_ratio, uid, iid, label)

    def per_pos_stratified_pointwise(self, seed, first, n, pos_ratio, uid, iid, label):
        """(user, item, label) samples [first, first + n) of `Dataset.per_pos_stratified_pointwise` into DEVICE buffers"""
        self._pointwise(self._lib.orx_sampler_per_pos_stratified, seed, first, n, pos_ratio, uid, iid, label)


Sampler = DeviceSampler


# ---- alternating least squares for WRMF (orx_als_half_step) ------------------------------------------------------------------
def als_segment_len():
    """orx_als_segment_len: rows of more entries than this are cut into segments whose partial sums are added in segment order"""
    return int(_ffi.load().orx_als_segment_len())


class ALSCsr:
    """One direction of an interaction set for `als_half_step`: row r observes the columns cols[ptr[r]:ptr[r + 1]] (ascending,
    distinct), with the confidences conf[...] aligned with cols, or None for one confidence `a` everywhere.  The host arrays are
    always there; `to_device(ctx)` adds copies in HBM (torch tensors) that the half-steps then read without any upload."""

    def __init__(self, ptr, cols, conf, n_cols):
        self.ptr = np.ascontiguousarray(ptr, np.int64)
        self.cols = np.ascontiguousarray(cols, np.int32)
        self.conf = None if conf is None else np.ascontiguousarray(conf, np.float32)
        if self.ptr.ndim != 1 or self.ptr.size < 1 or self.ptr[0] != 0 or np.any(np.diff(self.ptr) < 0) or self.ptr[-1] != self.cols.size:
            raise ValueError("ALSCsr: ptr must start at 0, never decrease and end at len(cols)")
        if self.conf is not None and self.conf.shape != self.cols.shape:
            raise ValueError("ALSCsr: conf must be aligned with cols")
        self.shape = (self.ptr.size - 1, int(n_cols))
        self._dev = None           # (ctx, ptr, cols, conf) device tensors

    @classmethod
    def from_pairs(cls, rows, cols, conf, n_rows, n_cols):
        """(row, col[, confidence]) records -> CSR; a repeated pair is one entry (as DeviceSampler merges them) whose confidence
        is the sum of its records'"""
        rows = np.asarray(rows, np.int64).reshape(-1); cols = np.asarray(cols, np.int64).reshape(-1)
        if rows.size and (rows.min() < 0 or rows.max() >= n_rows or cols.min() < 0 or cols.max() >= n_cols):
            raise IndexError(f"ALS data: an id outside [0, {n_rows}) x [0, {n_cols})")
        key, inv = np.unique(rows * int(n_cols) + cols, return_inverse=True)       # sorted by (row, col), distinct
        ptr = np.zeros(int(n_rows) + 1, np.int64)
        np.cumsum(np.bincount(key // int(n_cols), minlength=int(n_rows)), out=ptr[1:])
        c = None
        if conf is not None:
            c = np.bincount(inv.reshape(-1), weights=np.asarray(conf, np.float64).reshape(-1), minlength=key.size).astype(np.float32)
        return cls(ptr, (key % int(n_cols)).astype(np.int32), c, n_cols)

    @property
    def on_device(self):
        return self._dev is not None

    def to_device(self, ctx=None):
        """a view of the same lists that als_half_step reads from HBM (needs torch)"""
        import torch
        ctx = ctx or default_context()
        dv = torch.device("cuda", ctx.device)
        out = ALSCsr.__new__(ALSCsr)
        out.ptr, out.cols, out.conf, out.shape = self.ptr, self.cols, self.conf, self.shape
        t = [torch.from_numpy(self.ptr).to(dv), torch.from_numpy(self.cols).to(dv),
             torch.from_numpy(self.conf).to(dv) if self.conf is not None else None]
        torch.cuda.current_stream(dv).synchronize()        # the copies are complete before the library's stream reads them
        out._dev = (ctx, *t)
        return out

    def to_host(self):
        """a view of the same lists that als_half_step uploads from the host arrays at every call"""
        out = ALSCsr.__new__(ALSCsr)
        out.ptr, out.cols, out.conf, out.shape, out._dev = self.ptr, self.cols, self.conf, self.shape, None
        return out


class ALSData:
    """An interaction set prepared for ALS: `by_user` (user -> items) and `by_item` (item -> users), each an ALSCsr, built once.
    `raw_data`: the structured array the reference's Dataset takes ('user_id', 'item_id'); repeated records are one observation.
    `confidence`: one float per record (the c_ui of Hu / Koren / Volinsky; records of one pair add up), or None for the model's
    `a` everywhere.  The lists are kept on the device when torch is there (device=False: host arrays only)."""

    def __init__(self, raw_data, total_users, total_items, confidence=None, ctx=None, device=True):
        self.ctx = ctx or default_context()
        u = np.asarray(raw_data["user_id"]); i = np.asarray(raw_data["item_id"])
        if confidence is not None:
            confidence = np.asarray(confidence, np.float64).reshape(-1)
            if confidence.size != u.size:
                raise ValueError(f"ALSData: {confidence.size} confidences for {u.size} records")
        self.total_users, self.total_items = int(total_users), int(total_items)
        self.by_user = ALSCsr.from_pairs(u, i, confidence, self.total_users, self.total_items)
        self.by_item = ALSCsr.from_pairs(i, u, confidence, self.total_items, self.total_users)
        self.nnz = int(self.by_user.cols.size)
        if device:
            try:
                import torch  # noqa: F401
            except ImportError:
                device = False
        if device:
            self.by_user, self.by_item = self.by_user.to_device(self.ctx), self.by_item.to_device(self.ctx)


def _als_rows(rows, n, what="als_half_step", table="the solved table"):
    if rows is None:
        return 0, n
    if isinstance(rows, range):
        if rows.step != 1:
            raise ValueError(f"{what}: rows must be a contiguous range")
        row0, nrows = (rows.start, len(rows)) if len(rows) else (0, 0)
    else:
        row0, nrows = (int(x) for x in rows)
    if row0 < 0 or nrows < 0 or row0 + nrows > n:
        raise ValueError(f"{what}: rows [{row0}, {row0 + nrows}) outside {table}'s {n} rows")
    return row0, nrows


_ALS_SOLVERS = ("cholesky", "cg")


def als_cg_row_breaks(dim):
    """orx_als_cg_row_breaks: the row lengths at which the CG half-step changes its code path for tables of this dim, ascending
    (entries kept in LDS / streamed per product / cut into segments across workgroups)"""
    out = np.zeros(8, np.int32)
    n = int(_ffi.load().orx_als_cg_row_breaks(int(dim), out.ctypes.data, out.size))
    return [int(x) for x in out[:min(n, out.size)]]


def _als_solver(what, solver, cg_steps):
    if solver not in _ALS_SOLVERS:
        raise ValueError(f"{what}: solver must be one of {_ALS_SOLVERS}, got {solver!r}")
    cg_steps = int(cg_steps)
    if not 1 <= cg_steps <= 128:
        raise ValueError(f"{what}: cg_steps = {cg_steps} outside [1, 128]")
    return cg_steps


def _als_check(what, one, other, csr, a, b, reg):
    """the argument rules the half-steps and the objective share -> (a, b, reg) as floats"""
    if not isinstance(csr, ALSCsr):
        raise ValueError(f"{what}: csr must be an ALSCsr (ALSData.by_user / .by_item)")
    if one is other or one._h.value == other._h.value:
        raise ValueError(f"{what}: fixed and solved are the same table")
    if one.ctx is not other.ctx:
        raise ValueError(f"{what}: the tables live on different contexts")
    if one.dim != other.dim:
        raise ValueError(f"{what}: fixed dim {one.dim}, solved dim {other.dim}")
    if not 1 <= one.dim <= 128:
        raise ValueError(f"{what}: dim {one.dim} outside [1, 128]")
    a, b, reg = float(a), float(b), float(reg)
    if not (np.isfinite(reg) and reg > 0):
        raise ValueError(f"{what}: reg must be finite and > 0, got {reg!r}")
    if not (np.isfinite(b) and b >= 0):
        raise ValueError(f"{what}: b must be finite and >= 0, got {b!r}")
    if csr.conf is None and not (np.isfinite(a) and a >= b):
        raise ValueError(f"{what}: a = {a!r} must be finite and >= b = {b!r}")
    if csr.shape != (other.rows, one.rows):
        raise ValueError(f"{what}: a CSR of shape {csr.shape} for tables of {other.rows} and {one.rows} rows")
    return a, b, reg


def _als_csr_args(what, csr, ctx):
    """-> (row_ptr, cols, conf, flags) as the library takes them"""
    if csr.on_device:
        dctx, ptr, cols, conf = csr._dev
        if dctx is not ctx:
            raise ValueError(f"{what}: the CSR was put on the device of another context")
        return ptr.data_ptr(), cols.data_ptr(), conf.data_ptr() if conf is not None else None, _ffi.ORX_IDS_DEVICE
    return csr.ptr.ctypes.data, csr.cols.ctypes.data, csr.conf.ctypes.data if csr.conf is not None else None, 0


def als_half_step(fixed, solved, csr, a=1.0, b=1.0, reg=0.1, rows=None, solver="cholesky", cg_steps=3):
    """One ALS half-step of WRMF: `fixed` stays, rows `rows` (None: all; a range or (row0, nrows)) of `solved` are overwritten
    with the exact minimisers of  sum_cells c (p - x.f)^2 + reg |x|^2  given `fixed` -- observed cells (csr: an ALSCsr over the
    rows of `solved` and the rows of `fixed` as columns) have preference 1 and confidence csr.conf, or `a` when it is None;
    all others preference 0 and confidence `b`.  No bias term.  x is a function of the row's own data alone: the same bits for
    any split into calls.  solver="cg" replaces the exact minimiser by `cg_steps` steps of conjugate gradient started from the
    row's current value (orx_als_half_step_cg): no factorisation, a descent step of the same objective (`als_objective`).
    Bad arguments raise ValueError before the library is called; a column outside `fixed` IndexError."""
    cg_steps = _als_solver("als_half_step", solver, cg_steps)
    a, b, reg = _als_check("als_half_step", fixed, solved, csr, a, b, reg)
    row0, nrows = _als_rows(rows, solved.rows)
    fixed._sync_pending(); solved._sync_pending()
    lib = fixed.ctx._lib
    ptr, cols, conf, flags = _als_csr_args("als_half_step", csr, fixed.ctx)
    if solver == "cg":
        check(lib.orx_als_half_step_cg(fixed.ctx._h, fixed._h, solved._h, ptr, cols, conf, row0, nrows, a, b, reg, cg_steps, flags))
    else:
        check(lib.orx_als_half_step(fixed.ctx._h, fixed._h, solved._h, ptr, cols, conf, row0, nrows, a, b, reg, flags))
    return solved


def als_sweep(user, item, data, a=1.0, b=1.0, reg=0.1, solver="cholesky", cg_steps=3):
    """One ALS sweep: the user half-step (items fixed), then the item half-step (users fixed).  `data`: an ALSData."""
    als_half_step(item, user, data.by_user, a, b, reg, solver=solver, cg_steps=cg_steps)
    als_half_step(user, item, data.by_item, a, b, reg, solver=solver, cg_steps=cg_steps)


def als_objective(user, item, data, a=1.0, b=1.0, reg=0.1):
    """What the half-steps descend, on the device (orx_als_objective):  sum over ALL cells c (p - u.v)^2 + reg (|U|_F^2 + |V|_F^2)
    from the two grams and one pass over the observations, reduced in fp64 in a fixed order (two calls give the same bits).
    `data`: an ALSData, or the user -> items ALSCsr.  Synchronises; -> float."""
    csr = data.by_user if isinstance(data, ALSData) else data
    a, b, reg = _als_check("als_objective", item, user, csr, a, b, reg)
    user._sync_pending(); item._sync_pending()
    ptr, cols, conf, flags = _als_csr_args("als_objective", csr, user.ctx)
    out = c_double()
    check(user.ctx._lib.orx_als_objective(user.ctx._h, user._h, item._h, ptr, cols, conf, a, b, reg, flags, byref(out)))
    return float(out.value)


# ---- graph propagation and LightGCN (orx_graph_spmm, orx_table_apply_dense, orx_lightgcn_*) ----------------------------------
LIGHTGCN_MAX_LAYERS = 8
_GRAPH_NORMS = ("sym", "none")


def graph_segment_len():
    """orx_graph_segment_len: rows of more entries than this are cut into segments, summed by separate wavefronts and added in
    segment order"""
    return int(_ffi.load().orx_graph_segment_len())


def graph_scales(csr):
    """the symmetric normalisation's scale of every row of `csr`, on the host in float32: 1 / sqrt(degree), exact 0 for degree 0
    (the bits are NumPy's, not a device rsqrt's)"""
    deg = np.diff(csr.ptr).astype(np.float32)
    out = np.zeros(deg.shape, np.float32)
    nz = deg > 0
    out[nz] = np.float32(1) / np.sqrt(deg[nz])
    return out


def graph_long_segments(csr):
    """the number of segments of the rows of `csr` that are longer than graph_segment_len(), sum of ceil(n / segment_len) over
    those rows: what orx_graph_spmm sizes its scratch of partial sums from when the CSR lives on the device (0: no row is cut,
    no plan and no segment launch).  Counted once from the host arrays and kept on the ALSCsr."""
    n = getattr(csr, "_graph_long", None)
    if n is None:
        S = graph_segment_len()
        deg = np.diff(csr.ptr)
        deg = deg[deg > S]
        n = csr._graph_long = int(((deg + S - 1) // S).sum())
    return n


class InteractionGraph:
    """The user-item graph of an interaction set, prepared for propagation: both CSRs of an `ALSData` (user -> items, item ->
    users) and the two scale vectors in HBM (needs torch).  `data_or_raw`: an ALSData, or the structured array ('user_id',
    'item_id') ALSData takes, with total_users / total_items.  norm="sym": edge (u, i) weighs 1 / sqrt(deg u . deg i), formed as
    a row scale times a column scale; norm="none": unit scales, a plain neighbour sum.  Confidences of the ALSCsr lists are
    IGNORED: every observed pair is one unweighted edge."""

    def __init__(self, data_or_raw, total_users=None, total_items=None, norm="sym", ctx=None):
        if norm not in _GRAPH_NORMS:
            raise ValueError(f"InteractionGraph: norm must be one of {_GRAPH_NORMS}, got {norm!r}")
        if isinstance(data_or_raw, ALSData):
            data = data_or_raw
            if ctx is not None and ctx is not data.ctx:
                raise ValueError("InteractionGraph: the ALSData lives on another context")
            if (total_users is not None and int(total_users) != data.total_users) or \
                    (total_items is not None and int(total_items) != data.total_items):
                raise ValueError("InteractionGraph: total_users / total_items differ from the ALSData's")
        else:
            if total_users is None or total_items is None:
                raise ValueError("InteractionGraph: raw records need total_users and total_items")
            data = ALSData(data_or_raw, total_users, total_items, ctx=ctx)
        self.data, self.ctx, self.norm = data, data.ctx, norm
        self.total_users, self.total_items, self.nnz = data.total_users, data.total_items, data.nnz
        self.by_user = data.by_user if data.by_user.on_device else data.by_user.to_device(self.ctx)
        self.by_item = data.by_item if data.by_item.on_device else data.by_item.to_device(self.ctx)
        self.user_scale_host = self.item_scale_host = None
        self.user_scale = self.item_scale = None
        if norm == "sym":
            import torch
            dv = torch.device("cuda", self.ctx.device)
            self.user_scale_host, self.item_scale_host = graph_scales(self.by_user), graph_scales(self.by_item)
            self.user_scale = torch.from_numpy(self.user_scale_host).to(dv)
            self.item_scale = torch.from_numpy(self.item_scale_host).to(dv)
            torch.cuda.current_stream(dv).synchronize()        # complete before the library's stream reads them

    def _scale_ptrs(self):
        if self.user_scale is None:
            return None, None
        return self.user_scale.data_ptr(), self.item_scale.data_ptr()


def _graph_scale_arg(what, name, x, n, ctx):
    """a scale vector -> (pointer or None, keepalive): a float32 device tensor of n entries, or a host array that is uploaded"""
    if x is None:
        return None, None
    if not _is_device_tensor(x):
        import torch
        h = np.ascontiguousarray(np.asarray(x), np.float32).reshape(-1)
        x = torch.from_numpy(h).to(torch.device("cuda", ctx.device))
        torch.cuda.current_stream(x.device).synchronize()
    if not str(x.dtype).endswith("float32") or x.numel() != n or not x.is_contiguous():
        raise ValueError(f"{what}: {name} must be {n} contiguous float32 values")
    ctx.after_torch(x)
    return x.data_ptr(), x


def _graph_check(what, X, out, acc, csr):
    if not isinstance(csr, ALSCsr):
        raise ValueError(f"{what}: csr must be an ALSCsr (InteractionGraph.by_user / .by_item)")
    tabs = [("X", X), ("out", out)] + ([("acc", acc)] if acc is not None else [])
    for i, (na, a) in enumerate(tabs):
        for nb, b in tabs[i + 1:]:
            if a is b or a._h.value == b._h.value:
                raise ValueError(f"{what}: {na} and {nb} are the same table")
    for name, t in tabs:
        if t.ctx is not X.ctx:
            raise ValueError(f"{what}: the tables live on different contexts")
        if t.dim != X.dim:
            raise ValueError(f"{what}: X dim {X.dim}, {name} dim {t.dim}")
    if not 1 <= X.dim <= 128:
        raise ValueError(f"{what}: dim {X.dim} outside [1, 128]")
    if acc is not None and acc.rows != out.rows:
        raise ValueError(f"{what}: acc has {acc.rows} rows, out {out.rows}")
    if csr.shape != (out.rows, X.rows):
        raise ValueError(f"{what}: a CSR of shape {csr.shape} for tables of {out.rows} and {X.rows} rows")


def graph_spmm(X, out, csr, row_scale=None, col_scale=None, rows=None, acc=None, acc_alpha=0.0, long_segments=None):
    """One half-layer of the graph propagation (orx_graph_spmm): for the rows `rows` (None: all; a range or (row0, nrows)) of
    `csr` -- an ALSCsr over the rows of `out` whose columns index the rows of `X` --
        out[r] = y[r] = row_scale[r] * sum_e col_scale[cols[e]] * X[cols[e]],      acc[r] += acc_alpha * y[r]  (acc given)
    row_scale / col_scale: float32 vectors over ALL rows of out / X (device tensors, or host arrays that are uploaded), None: 1.
    An empty row writes +0.0 and leaves acc alone.  y[r] has the same bits for any row range, split into calls, other rows in the
    call, and a host or device CSR; no float atomics.  long_segments: None (counted from the CSR: graph_long_segments), or the
    number of scratch slots the partial sums of rows longer than graph_segment_len() may take with a device CSR -- a long row
    that finds no slot walks its segments itself and gives the same bits, only more slowly.  Bad arguments raise ValueError
    before the library is called; a column outside `X` IndexError."""
    _graph_check("graph_spmm", X, out, acc, csr)
    row0, nrows = _als_rows(rows, out.rows, "graph_spmm", "out")
    long_segments = graph_long_segments(csr) if long_segments is None else int(long_segments)
    if long_segments < 0:
        raise ValueError(f"graph_spmm: long_segments = {long_segments}")
    ps, k0 = _graph_scale_arg("graph_spmm", "row_scale", row_scale, out.rows, X.ctx)
    pc, k1 = _graph_scale_arg("graph_spmm", "col_scale", col_scale, X.rows, X.ctx)
    for t in (X, out, acc):
        if t is not None:
            t._sync_pending()
    ptr, cols, _, flags = _als_csr_args("graph_spmm", csr, X.ctx)
    check(X.ctx._lib.orx_graph_spmm(X.ctx._h, X._h, out._h, acc._h if acc is not None else None, float(acc_alpha), ptr, cols, ps, pc,
                                    row0, nrows, long_segments, flags))
    if flags:
        X.ctx.check_index_error()
    return out


def table_apply_dense(opt, table, grad):
    """orx_table_apply_dense: the Keras dense rule of `opt` (SGD, momentum / Nesterov, Adagrad, Adam) on every element of `table`
    with the gradient `grad` -- a float32 device tensor or a Table of the table's shape, read only.  Adam's counter advances by
    one; a lazily-applied Adam on the table is finished first, so the table can go to pairwise_step and back."""
    if isinstance(grad, Table):
        if grad is table or grad.ctx is not table.ctx or (grad.rows, grad.dim) != (table.rows, table.dim):
            raise ValueError("table_apply_dense: grad must be another table of the same context and shape")
        grad._sync_pending()
        gp = grad.device_ptr
    else:
        if not _is_device_tensor(grad) or not str(grad.dtype).endswith("float32") or not grad.is_contiguous() or \
                grad.numel() != table.rows * table.dim:
            raise ValueError(f"table_apply_dense: grad must be a contiguous float32 device tensor of {table.rows} x {table.dim} values")
        table.ctx.after_torch(grad)
        gp = grad.data_ptr()
    table._sync_pending()
    check(table.ctx._lib.orx_table_apply_dense(table.ctx._h, opt._h, table._h, gp))
    _keep_tables(opt, (table,))
    return table


class LightGCN:
    """LightGCN (He et al., SIGIR 2020) over the trainable tables U [users, D] and V [items, D] and an InteractionGraph:
        E(0) = [U ; V],  E(k+1) = A~ E(k),  E_f = sum_k layer_weights[k] E(k)        (layer_weights: 1 / (layers + 1) by default)
    The rows that are scored are E_f's.  `propagate()` gives them as two Tables that recommend_topk, rank_metrics_matrixfree,
    score_candidates and the samplers take as they stand; `step` is one BPR step (no item bias) through the propagation."""

    def __init__(self, U, V, graph, layers=3, layer_weights=None, bias=None):
        what = "LightGCN"
        if bias is not None:
            raise ValueError(f"{what}: the model has no item bias (a bias table was passed)")
        if not isinstance(graph, InteractionGraph):
            raise ValueError(f"{what}: graph must be an InteractionGraph")
        layers = int(layers)
        if not 1 <= layers <= LIGHTGCN_MAX_LAYERS:
            raise ValueError(f"{what}: layers = {layers} outside [1, {LIGHTGCN_MAX_LAYERS}]")
        if layer_weights is not None:
            layer_weights = np.ascontiguousarray(np.asarray(layer_weights, np.float32).reshape(-1))
            if layer_weights.size != layers + 1:
                raise ValueError(f"{what}: {layer_weights.size} layer weights for {layers} layers (one per layer and one for layer 0)")
        if U is V or U._h.value == V._h.value:
            raise ValueError(f"{what}: the user and the item table are the same table")
        if U.ctx is not V.ctx or graph.ctx is not U.ctx:
            raise ValueError(f"{what}: the tables and the graph live on different contexts")
        if U.dim != V.dim:
            raise ValueError(f"{what}: user dim {U.dim}, item dim {V.dim}")
        if not 1 <= U.dim <= 128:
            raise ValueError(f"{what}: dim {U.dim} outside [1, 128]")
        if (graph.total_users, graph.total_items) != (U.rows, V.rows):
            raise ValueError(f"{what}: a graph of {graph.total_users} x {graph.total_items} for tables of {U.rows} and {V.rows} rows")
        self.U, self.V, self.graph, self.ctx = U, V, graph, U.ctx
        self.layers = layers
        self.layer_weights = layer_weights if layer_weights is not None else np.full(layers + 1, np.float32(1) / np.float32(layers + 1), np.float32)
        _, up, uc, _ = graph.by_user._dev
        _, ip, ic, _ = graph.by_item._dev
        su, sv = graph._scale_ptrs()
        h = c_void_p()
        lib = self.ctx._lib
        check(lib.orx_lightgcn_create(self.ctx._h, U._h, V._h, up.data_ptr(), uc.data_ptr(), ip.data_ptr(), ic.data_ptr(), su, sv,
                                      graph_long_segments(graph.by_user), graph_long_segments(graph.by_item), layers, self.layer_weights.ctypes.data, byref(h)))
        self._h = h
        self._keep = (U, V, graph)
        self._fin = weakref.finalize(self, lib.orx_lightgcn_destroy, h)
        hu, hv = c_void_p(), c_void_p()
        check(lib.orx_lightgcn_tables(h, byref(hu), byref(hv)))
        self.Uf, self.Vf = _BorrowedTable(self.ctx, hu, self), _BorrowedTable(self.ctx, hv, self)
        self._fresh = False

    def invalidate(self):
        """U or V were changed by anything but this object's own `step` (rt.pairwise_step, rt.table_apply_dense, Table.write,
        a checkpoint load ...): the next propagate() recomputes.  Nothing else tells the object: without this call propagate()
        goes on returning the tables of the last propagation."""
        self._fresh = False

    def propagate(self, force=False):
        """-> (Uf, Vf), the propagated tables (valid until the next step); recomputed when `step` has run since, when
        `invalidate()` was called, or with force=True.  A change of U or V from OUTSIDE this object (rt.pairwise_step,
        rt.table_apply_dense, Table.write) is not seen: call invalidate() after it, or pass force=True."""
        if force or not self._fresh:
            self.U._sync_pending(); self.V._sync_pending()
            check(self.ctx._lib.orx_lightgcn_propagate(self._h))
            self._fresh = True
        return self.Uf, self.Vf

    def _args(self, what, uid, pid, nid):
        """-> B, the flag word, the three pointers, the keepalives; U and V are flushed"""
        _, B, _, dev, (pu, pp, pn, _), keep = _triplet_args(what, uid, pid, nid)
        self.ctx.after_torch(*keep)
        self.U._sync_pending(); self.V._sync_pending()
        return B, _flags(dev), (pu, pp, pn), keep

    def step(self, opt, uid, pid, nid, l2_reg=0.0, train=None, want_loss=True):
        """One train step on the triplets (uid, pid, nid): loss = mean -log sigmoid(s_p - s_n) on the propagated rows plus
        l2_reg / B * sum (|U[u]|^2 + |V[p]|^2 + |V[n]|^2) / 2 on the layer-0 rows; the dense rule of `opt` on U and V (train:
        None, or ("user",) / ("item",) to leave the other table bit for bit as it is).  -> (loss, l2) as floats when want_loss,
        else None (no host synchronisation with device ids).  Bit-reproducible."""
        what = "LightGCN.step"
        mask = _train_mask(train, None, what)
        l2_reg = _coef_arg(what, "l2_reg", l2_reg)
        B, flags, ptrs, keep = self._args(what, uid, pid, nid)
        loss, l2 = ctypes.c_float(), ctypes.c_float()
        self._fresh = False
        check(self.ctx._lib.orx_lightgcn_step(self._h, opt._h, *ptrs, B, l2_reg, mask or 0, flags,
                                              byref(loss) if want_loss else None, byref(l2) if want_loss else None))
        _keep_tables(opt, (self.U, self.V))
        if flags and want_loss:
            self.ctx.check_index_error()
        return (float(loss.value), float(l2.value)) if want_loss else None

    def loss(self, uid, pid, nid, l2_reg=0.0):
        """the forward alone -> (loss, l2); U and V do not change (the propagated tables are brought up to date)"""
        what = "LightGCN.loss"
        l2_reg = _coef_arg(what, "l2_reg", l2_reg)
        B, flags, ptrs, keep = self._args(what, uid, pid, nid)
        loss, l2 = ctypes.c_float(), ctypes.c_float()
        check(self.ctx._lib.orx_lightgcn_loss(self._h, *ptrs, B, l2_reg, flags, byref(loss), byref(l2)))
        if flags:
            self.ctx.check_index_error()
        self._fresh = True
        return float(loss.value), float(l2.value)


# ---- VBPR: item content features through a learned projection (api_vbpr.hip) ----------------------------------------------------
class ItemFeatures:
    """Fixed fp32 item features F [items, Fd] in HBM: data, never trained.  A C-contiguous float32 NumPy array is uploaded once; a
    float32 torch device tensor is wrapped without a copy and kept alive.  `.rows`, `.dim`."""

    def __init__(self, array, ctx=None):
        what = "ItemFeatures"
        if _is_device_tensor(array):
            if array.dim() != 2 or not str(array.dtype).endswith("float32") or not array.is_contiguous():
                raise ValueError(f"{what}: a device tensor must be a contiguous float32 matrix [items, Fd]")
            self.rows, self.dim = int(array.shape[0]), int(array.shape[1])
            self._check_shape(what)
            self.ctx = ctx or default_context()
            self._tensor, self._table = array, None
            self.ctx.after_torch(array)
            self._ptr = int(array.data_ptr())
        else:
            a = np.asarray(array)
            if a.ndim != 2 or a.dtype != np.float32 or not a.flags.c_contiguous:
                raise ValueError(f"{what}: expected a C-contiguous float32 matrix [items, Fd], got {a.dtype} {list(a.shape)}")
            self.rows, self.dim = int(a.shape[0]), int(a.shape[1])
            self._check_shape(what)
            self.ctx = ctx or default_context()
            self._tensor, self._table = None, Table(self.rows, self.dim, self.ctx).write(a)
            self._ptr = int(self._table.device_ptr)

    def _check_shape(self, what):
        if self.rows < 1:
            raise ValueError(f"{what}: no item rows")
        if not 1 <= self.dim <= 8192:
            raise ValueError(f"{what}: feature dim Fd = {self.dim} outside [1, 8192]")

    @property
    def device_ptr(self):
        return self._ptr

    def write_rows(self, rows, values):
        """F[rows] = values (float32 [len(rows), Fd]): the features of newly arrived items"""
        rows = np.asarray(rows, np.int64).reshape(-1)
        vals = np.ascontiguousarray(values, np.float32).reshape(-1, self.dim)
        if vals.shape[0] != rows.size:
            raise ValueError(f"ItemFeatures.write_rows: {vals.shape[0]} rows of values for {rows.size} row ids")
        if rows.size and (rows.min() < 0 or rows.max() >= self.rows):
            raise IndexError(f"ItemFeatures.write_rows: a row outside [0, {self.rows})")
        if self._table is not None:
            for r, v in zip(rows, vals):
                self._table.write(v, row0=int(r))
        else:
            import torch
            self.ctx.synchronize()                 # (steps already queued on the library's stream read the rows as they were)
            self._tensor[torch.as_tensor(rows, device=self._tensor.device)] = torch.as_tensor(vals, device=self._tensor.device)
            self.ctx.after_torch(self._tensor)

    def read(self):
        return self._table.read() if self._table is not None else self._tensor.cpu().numpy()


def vbpr_geometry(B, Fd, Dc, batch_chunk=0):
    """what the launcher of the projection gradient does for (B, Fd, Dc, batch_chunk): a dict of the rows of the batch per chunk, the
    chunks, Dc padded to the tile width and the rows of E per workgroup.  No device is needed."""
    out = (c_int32 * 4)()
    check(_ffi.load().orx_vbpr_geometry(int(B), int(Fd), int(Dc), int(batch_chunk), out))
    return dict(chunk_rows=int(out[0]), chunks=int(out[1]), dim=int(out[2]), tile_rows=int(out[3]))


def _vbpr_check_proj(what, features, E):
    if not isinstance(features, ItemFeatures):
        raise ValueError(f"{what}: features must be an ItemFeatures")
    if features.ctx is not E.ctx:
        raise ValueError(f"{what}: the features and the projection live on different contexts")
    if E.rows != features.dim:
        raise ValueError(f"{what}: the projection has {E.rows} rows for features of dim {features.dim}")
    if E.dim < 1:
        raise ValueError(f"{what}: projection width Dc = {E.dim}; Dc must be in [1, 128]")
    if E.dim > 128:
        raise ValueError(f"{what}: projection width Dc = {E.dim} above 128")


def features_project(features, E, out_table, ids=None, minus=None, rows=None, col0=0):
    """out_table[k, col0 : col0 + Dc] = (F[ids[k]] - F[minus[k]]) E (orx_features_project).  minus=None: no subtraction; ids=None:
    the rows (row0, n) given by `rows` (default: all).  Row k of out_table is written, its other columns are not touched.  ids and
    minus live both on the host or both on the device.  -> out_table"""
    what = "features_project"
    _vbpr_check_proj(what, features, E)
    if out_table.ctx is not E.ctx:
        raise ValueError(f"{what}: the output table lives on a different context")
    col0 = int(col0)
    if col0 < 0 or col0 + E.dim > out_table.dim:
        raise ValueError(f"{what}: columns [{col0}, {col0 + E.dim}) do not fit a table of dim {out_table.dim}")
    pa = pb = None
    dev = False
    keep = []
    if ids is not None:
        if rows is not None:
            raise ValueError(f"{what}: ids together with rows")
        pa, n, dev, k0 = _ids_arg(ids)
        keep.append(k0)
        row0 = 0
    else:
        row0, n = (0, features.rows) if rows is None else (int(rows[0]), int(rows[1]))
        if row0 < 0 or n < 0 or row0 + n > features.rows:
            raise ValueError(f"{what}: rows ({row0}, {n}) outside the {features.rows} feature rows")
    if minus is not None:
        pb, nb, db, k1 = _ids_arg(minus)
        keep.append(k1)
        if ids is not None and db != dev:
            raise ValueError(f"{what}: ids and minus must be both on the host or both on the device")
        if nb != n:
            raise ValueError(f"{what}: {nb} ids in minus for {n} rows")
        dev = db
    if n > out_table.rows:
        raise ValueError(f"{what}: {n} rows for an output table of {out_table.rows}")
    E._sync_pending(); out_table._sync_pending()
    E.ctx.after_torch(ids, minus)
    check(E.ctx._lib.orx_features_project(E.ctx._h, features.device_ptr, features.rows, features.dim, E._h, pa, pb, row0, n,
                                          out_table.device_ptr, out_table.dim, col0, _ffi.ORX_IDS_DEVICE if dev else 0))
    return out_table


_VBPR_ROLES = dict(_TRAIN_ROLES, proj=_ffi.ORX_TRAIN_PROJ)


class VBPR:
    """VBPR (He & McAuley, AAAI 2016): BPR whose item vector is the latent row V[i] beside theta_i = F[i] E, a learned projection
    (no output bias, no activation) of a fixed feature row:
        s(u, i) = U[u, :Dl] . V[i] + U[u, Dl:] . (F[i] E) + b[i]
    U [users, Dl + Dc], V [items, Dl], b [items, 1] or None, E [Fd, Dc] (a Table like the others), features an ItemFeatures.
    `step` trains, `item_table()` gives [V | F E] as a Table that recommend_topk, rank_metrics_matrixfree, score_candidates and the
    samplers take with U and b as they stand."""

    def __init__(self, U, V, b, E, features):
        what = "VBPR"
        _vbpr_check_proj(what, features, E)
        if not (U.ctx is V.ctx is E.ctx) or (b is not None and b.ctx is not U.ctx):
            raise ValueError(f"{what}: the tables live on different contexts")
        if V.dim < 1:
            raise ValueError(f"{what}: latent dim {V.dim}")
        if V.dim + E.dim > 256:
            raise ValueError(f"{what}: D = Dl + Dc = {V.dim} + {E.dim} above 256")
        if U.dim != V.dim + E.dim:          # (said in VBPR's own words, ahead of _dot_tables' same test)
            raise ValueError(f"{what}: user dim {U.dim} != item latent dim {V.dim} + projection width {E.dim}")
        if features.rows != V.rows:
            raise ValueError(f"{what}: {features.rows} feature rows for {V.rows} items")
        _dot_tables(what, U.dim, V.dim + E.dim, V.rows, b)
        self.U, self.V, self.b, self.E, self.features, self.ctx = U, V, b, E, features, U.ctx
        self._W = None
        self._fresh = False

    def _args(self, what, uid, pid, nid, K, B, id_stride, weights):
        K, B, id_stride, dev, ptrs, keep = _triplet_args(what, uid, pid, nid, weights, K, B, id_stride)
        if B >= 2 ** 31 - 256:
            raise ValueError(f"{what}: B = {B}; B must be below 2^31 - 256")
        self.ctx.after_torch(*keep)
        for t in (self.U, self.V, self.b, self.E):
            if t is not None:
                t._sync_pending()
        return K, B, id_stride, dev, ptrs, keep

    def step(self, opt, uid, pid, nid, weights=None, l2_reg=0.0, l2_proj=0.0, train=None, K=1, B=None, id_stride=None,
             batch_chunk=0, want_loss=True):
        """K train steps (orx_vbpr_step) on the triplets: J = loss + l2_reg * l2_loss + l2_proj / 2 |E|^2.  weights: per-triplet
        weights shaped like the ids, living where they live.  train: None, or a subset of ("user", "item", "bias", "proj") -- every
        other table is read, never written.  batch_chunk: rows of the batch per partial sum of the projection gradient (0: the
        launcher's choice; else a positive multiple of 64).  -> (loss[K], l2[K]) as numpy float32, l2 the unscaled l2_loss of the
        rows, when want_loss, else None (no host synchronisation with device ids).  Bad arguments raise ValueError before the
        library is called; an id outside its table IndexError."""
        what = "VBPR.step"
        mask = _mask_arg(what, train, _VBPR_ROLES, self.b is not None) or 0
        l2_reg, l2_proj = _coef_arg(what, "l2_reg", l2_reg), _coef_arg(what, "l2_proj", l2_proj)
        batch_chunk = int(batch_chunk)
        if batch_chunk < 0 or batch_chunk % 64:
            raise ValueError(f"{what}: batch_chunk = {batch_chunk}; 0 (the launcher's choice) or a positive multiple of 64")
        K, B, id_stride, dev, ptrs, keep = self._args(what, uid, pid, nid, K, B, id_stride, weights)
        out, lp, l2p = _loss_outputs(K, want_loss)
        self._fresh = False
        f = self.features
        check(self.ctx._lib.orx_vbpr_step(self.ctx._h, opt._h, self.U._h, self.V._h, _bias_h(self.b), self.E._h, f.device_ptr, f.rows, f.dim,
                                          *ptrs, K, B, id_stride, l2_reg, l2_proj, batch_chunk, mask, _flags(dev), lp, l2p))
        _keep_tables(opt, (self.U, self.V, self.b, self.E))
        return out

    def loss(self, uid, pid, nid, weights=None):
        """forward only: (loss, l2_loss) of one batch -- the step's own numbers bit for bit on the same tables; no table changes"""
        _, B, _, dev, ptrs, keep = self._args("VBPR.loss", uid, pid, nid, 1, None, None, weights)
        out, lp, l2p = _loss_outputs(1, True)
        f = self.features
        check(self.ctx._lib.orx_vbpr_loss(self.ctx._h, self.U._h, self.V._h, _bias_h(self.b), self.E._h, f.device_ptr, f.rows, f.dim,
                                          *ptrs, B, _flags(dev), lp, l2p))
        return _loss_pair(out)

    def invalidate(self):
        """V, E or the features were changed by anything but this object's own `step` (another train step, Table.write, a
        checkpoint load ...): the next item_table() rebuilds.  Nothing else tells the object."""
        self._fresh = False

    def item_table(self, rows=None):
        """-> the Table [items, Dl + Dc] = [V | F E], owned by this object and valid until the next call.  It is rebuilt when a
        `step` has run since the last build or after invalidate(); rows=(row0, n) refreshes those rows only (newly arrived items)."""
        what = "VBPR.item_table"
        if self._W is None:
            self._W = Table(self.V.rows, self.U.dim, self.ctx)
            self._fresh = False
        f = self.features
        todo = None
        if not self._fresh:
            todo = (0, self.V.rows)
        elif rows is not None:
            todo = (int(rows[0]), int(rows[1]))
            if todo[0] < 0 or todo[1] < 0 or todo[0] + todo[1] > self.V.rows:
                raise ValueError(f"{what}: rows {todo} outside the {self.V.rows} items")
        if todo is not None:
            self.V._sync_pending(); self.E._sync_pending()
            check(self.ctx._lib.orx_vbpr_item_table(self.ctx._h, self.V._h, self.E._h, f.device_ptr, f.rows, f.dim, todo[0], todo[1],
                                                    self._W._h))
            self._fresh = True
        return self._W


# ---- history-pooled sequence recommender (orx_bag_pool / orx_seqrec_step / orx_seqrec_loss) -----------------------------------
_SEQ_ROLES = {"history": _ffi.ORX_TRAIN_USER, "item": _ffi.ORX_TRAIN_ITEM, "bias": _ffi.ORX_TRAIN_BIAS}


def _pool_arg(what, pool):
    """pool: "mean" | "sum" | ("fixed", denom) -> (orx_bag_mode, denom)"""
    if isinstance(pool, str):
        if pool == "mean":
            return _ffi.ORX_BAG_MEAN, 1.0
        if pool == "sum":
            return _ffi.ORX_BAG_FIXED, 1.0
    elif isinstance(pool, (tuple, list)) and len(pool) == 2 and pool[0] == "fixed":
        try:
            denom = float(pool[1])
        except (TypeError, ValueError):
            denom = float("nan")
        if not (np.isfinite(denom) and denom > 0.0):
            raise ValueError(f"{what}: pool = ('fixed', denom) needs a finite denom > 0 (got {pool[1]!r})")
        return _ffi.ORX_BAG_FIXED, denom
    raise ValueError(f"{what}: unknown pool {pool!r}; expected 'mean', 'sum' or ('fixed', denom)")


def bags_to_ragged(seq, seq_len):
    """The padded pair of the reference's samplers -- seq [B, L] item ids, seq_len [B] -- as ragged lists (ptr int32 [B + 1],
    items int32 [n]): bag i is seq[i, :seq_len[i]].  Positions t >= seq_len[i] are never read, whatever they hold.  NumPy in,
    NumPy out; torch device tensors in, device tensors out (one host synchronisation: n is a data-dependent size)."""
    what = "bags_to_ragged"
    if _is_device_tensor(seq) or _is_device_tensor(seq_len):
        import torch
        if not (_is_device_tensor(seq) and _is_device_tensor(seq_len)):
            raise ValueError(f"{what}: seq and seq_len must both be on the host or both on the device")
        if seq.dim() != 2 or seq_len.dim() != 1 or seq_len.shape[0] != seq.shape[0]:
            raise ValueError(f"{what}: seq {tuple(seq.shape)} and seq_len {tuple(seq_len.shape)}; expected [B, L] and [B]")
        L = seq.shape[1]
        ln = seq_len.to(torch.int64).clamp(0, L)
        mask = torch.arange(L, device=seq.device)[None, :] < ln[:, None]
        items = seq[mask].to(torch.int32).contiguous()
        ptr = torch.zeros(seq.shape[0] + 1, dtype=torch.int64, device=seq.device)
        ptr[1:] = torch.cumsum(ln, 0)
        return ptr.to(torch.int32).contiguous(), items
    seq = np.asarray(_host_array(seq))
    ln = np.asarray(_host_array(seq_len)).astype(np.int64).reshape(-1)
    if seq.ndim != 2 or ln.shape[0] != seq.shape[0]:
        raise ValueError(f"{what}: seq {seq.shape} and seq_len {ln.shape}; expected [B, L] and [B]")
    L = seq.shape[1]
    if ln.size and (ln.min() < 0 or ln.max() > L):
        raise ValueError(f"{what}: seq_len outside [0, {L}]")
    if ln.sum() >= 2 ** 31:
        raise ValueError(f"{what}: {int(ln.sum())} list entries; n must be below 2^31")
    mask = np.arange(L)[None, :] < ln[:, None]
    items = np.ascontiguousarray(seq[mask], dtype=np.int32)
    ptr = np.zeros(seq.shape[0] + 1, np.int32)
    ptr[1:] = np.cumsum(ln)
    return ptr, items


def _flat_keep(keep):
    """the arrays of a (possibly nested) keepalive tuple, for Context.after_torch"""
    out = []
    for k in keep:
        if isinstance(k, (tuple, list)):
            out.extend(_flat_keep(k))
        else:
            out.append(k)
    return out


def _host_array(x):
    return x.numpy() if hasattr(x, "numpy") and not isinstance(x, np.ndarray) else x


def _bags_arg(what, bags):
    """bags: (ptr [B + 1], items [n]) -- ragged, no host synchronisation wherever it lives -- or the padded pair (seq [B, L],
    seq_len [B]), converted here (padded input on the device costs one host synchronisation).
    -> (ptr pointer, items pointer, B, n, on_device, keepalive); a host ptr that breaks the contract is a ValueError here"""
    if not isinstance(bags, (tuple, list)) or len(bags) != 2:
        raise ValueError(f"{what}: bags must be (ptr, items) or the padded pair (seq [B, L], seq_len [B])")
    first, second = bags
    shape = tuple(getattr(first, "shape", ())) if not isinstance(first, DevicePtr) else ()
    if len(shape) == 2:
        first, second = bags_to_ragged(first, second)
    pp, npn, dp, k0 = _ids_arg(first)
    pi, n, di, k1 = _ids_arg(second)
    if dp != di:
        raise ValueError(f"{what}: bags must be all on the host or all on the device")
    if npn < 1:
        raise ValueError(f"{what}: bag offsets need B + 1 entries (got {npn})")
    B = npn - 1
    if n >= 2 ** 31:
        raise ValueError(f"{what}: {n} list entries; n must be below 2^31")
    if not dp:
        ptr = k0
        if ptr[0] != 0 or (B and (np.diff(ptr) < 0).any()) or ptr[B] != n:
            raise ValueError(f"{what}: bag offsets must start at 0, never decrease and end at n = {n} "
                             f"(got ptr[0] = {int(ptr[0])}, ptr[B] = {int(ptr[B])}"
                             f"{', decreasing' if B and (np.diff(ptr) < 0).any() else ''})")
    return pp, pi, B, n, dp, (k0, k1, first, second)


def _seqrec_check_tables(what, H, V, b):
    if H is V:
        raise ValueError(f"{what}: the history table and the item table are the same table (tied tables are not offered)")
    if H.ctx is not V.ctx or (b is not None and b.ctx is not H.ctx):
        raise ValueError(f"{what}: the tables live on different contexts")
    if (H.rows, H.dim) != (V.rows, V.dim):          # (rows too: the history table is indexed by item)
        raise ValueError(f"{what}: history table [{H.rows}, {H.dim}] and item table [{V.rows}, {V.dim}] differ in shape")
    if H.dim > 256:
        raise ValueError(f"{what}: dim {H.dim} above 256")
    _dot_tables(what, H.dim, V.dim, V.rows, b)


def _labels_arg(what, pid, labels, label_weights, dev, B):
    """the label part of a full-softmax call: one label per bag (pid) or a label set per bag (labels: (ptr, items) or the padded
    pair (seq, seq_len), as _bags_arg takes bags; label_weights: one float per ragged entry, or [B, L] beside a padded pair).
    -> (the C arguments between the bags and the weights, sets?, keepalive)"""
    if (pid is None) == (labels is None):
        raise ValueError(f"{what}: pass either pid (one label per bag) or labels (a label set per bag), "
                         f"{'not both' if pid is not None else 'one of them'}")
    if labels is None:
        if label_weights is not None:
            raise ValueError(f"{what}: label_weights without labels")
        (ppid,), (npid,), _, keep = _id_lists(what, (pid,), dev)          # (on the side the bags are on)
        if npid != B:
            raise ValueError(f"{what}: {B} bags and {npid} label ids (one label per bag)")
        return (ppid,), False, keep
    if not isinstance(labels, (tuple, list)) or len(labels) != 2:
        raise ValueError(f"{what}: labels must be (ptr, items) or the padded pair (seq [B, L], seq_len [B])")
    shape = tuple(getattr(labels[0], "shape", ())) if not isinstance(labels[0], DevicePtr) else ()
    if len(shape) == 2 and label_weights is not None:                   # padded weights follow their padded ids
        if tuple(getattr(label_weights, "shape", ())) != shape:
            raise ValueError(f"{what}: label_weights {list(getattr(label_weights, 'shape', ()))} beside padded labels {list(shape)}")
        if _is_device_tensor(labels[0]):
            import torch
            if not _is_device_tensor(label_weights):
                raise ValueError(f"{what}: label_weights on the host with labels on the device (label_weights lives where the ids live)")
            ln = labels[1].to(torch.int64).clamp(0, shape[1])
            label_weights = label_weights[torch.arange(shape[1], device=labels[0].device)[None, :] < ln[:, None]].float().contiguous()
        else:
            ln = np.asarray(_host_array(labels[1])).astype(np.int64).reshape(-1)
            lw = np.asarray(_host_array(label_weights), dtype=np.float32)
            label_weights = np.ascontiguousarray(lw[np.arange(shape[1])[None, :] < ln[:, None]])
    lp, li, LB, n_lab, ldev, kl = _bags_arg(what + " labels", labels)
    if ldev != dev:
        raise ValueError(f"{what}: the label sets must live where the bags live")
    if LB != B:
        raise ValueError(f"{what}: {B} bags and {LB} label sets (one set per bag)")
    ptw, ktw = _floats_arg(what, "label_weights", label_weights, dev, n_lab, "the label entries")
    return (lp, li, ptw, n_lab), True, (kl, ktw)


# What SeqRec.step_full / loss_full and DeepSeqRec.step_full / loss_full share (4.5z has the C side).  m: the model
# (H, V, b, ctx, _mode, _denom); lists(what) reads the model's own lists -> (bag ptr, bag items, B, n, on_device, a callable that
# makes the model's C arguments between the bias and the bags -- called last, after every refusal --, keepalives); tables: what
# the call flushes and the optimizer keeps; fns: the C functions' names (one label per bag, a label set per bag); coefs:
# l2_reg [, l2_mlp] as checked by the caller.
def _full_args(what, m, lists, tables, pid, weights, item_offset, scale, chunk_items, chunk_samples, labels, label_weights):
    scale = _scale_arg(what, scale)
    ci, cs = _chunk_arg(what, "chunk_items", chunk_items), _chunk_arg(what, "chunk_samples", chunk_samples)
    pp, pi, B, n, dev, model, kl = lists(what)
    plab, sets, keep = _labels_arg(what, pid, labels, label_weights, dev, B)
    pw, kw = _floats_arg(what, "weights", weights, dev, B, "the bags")
    po, ko = _floats_arg(what, "item_offset", item_offset, dev, m.V.rows, "the item table's rows")
    m.ctx.after_torch(*_flat_keep(kl), *_flat_keep(keep), kw, ko)
    for t in tables:
        if t is not None:
            t._sync_pending()
    return B, n, dev, sets, (*model(), pp, pi, *plab, pw, po), scale, ci, cs, (kl, keep, kw, ko)


def _full_step(what, m, fns, lists, tables, opt, coefs, mask, pid, weights, item_offset, scale, chunk_items, chunk_samples, want_loss, labels,
               label_weights):
    B, n, dev, sets, ptrs, scale, ci, cs, keep = _full_args(what, m, lists, tables, pid, weights, item_offset, scale, chunk_items, chunk_samples,
                                                            labels, label_weights)
    out, lp, l2p = _loss_outputs(1, want_loss)
    check(getattr(m.ctx._lib, fns[sets])(m.ctx._h, opt._h, m.H._h, m.V._h, _bias_h(m.b), *ptrs, B, n, m._mode, m._denom, scale, *coefs, ci, cs,
                                         mask, _flags(dev), lp, l2p))
    _keep_tables(opt, tables)
    return out


def _full_loss(what, m, fns, lists, tables, pid, weights, item_offset, scale, chunk_items, per_row, labels, label_weights):
    B, n, dev, sets, ptrs, scale, ci, _, keep = _full_args(what, m, lists, tables, pid, weights, item_offset, scale, chunk_items, 0, labels,
                                                           label_weights)
    out, lp, l2p = _loss_outputs(1, True)
    rows, rp = _row_loss_buffer(m.ctx, B, dev, per_row)
    check(getattr(m.ctx._lib, fns[sets])(m.ctx._h, m.H._h, m.V._h, _bias_h(m.b), *ptrs, B, n, m._mode, m._denom, scale, ci, _flags(dev), lp, l2p, rp))
    return _forward_result(out, rows, dev)


def _owned_output(what, m, B, dim, out, rows_are="bags"):
    """the output table of a user_table call: `out` once its shape is checked, or the one the model owns -- valid until the
    next call with another B"""
    if B < 1:
        raise ValueError(f"{what}: no bags")
    if out is None:
        if m._Q is None or m._Q.rows != B:
            m._Q = Table(B, dim, m.ctx)
        return m._Q
    if (out.rows, out.dim) != (B, dim):
        raise ValueError(f"{what}: out is [{out.rows}, {out.dim}] for {B} {rows_are} of dim {dim}")
    return out


def bag_pool(H, bags, out, pool="mean", rows=None):
    """out[row0 + i] = c_i * sum of H[items of bag i] in list order (orx_bag_pool): an EmbeddingBag over per-call ragged lists.
    bags: (ptr, items) or the padded pair (seq, seq_len) -- see _bags_arg; pool: "mean" (c_i = 1 / len_i), "sum", or
    ("fixed", denom) (c_i = 1 / denom).  rows: (row0, B) of `out` to write (None: (0, B)); `out` is another Table of H's dim and
    nothing else of it is touched.  An empty bag pools to +0.  Bad arguments raise ValueError before the library is called; an id
    outside H raises IndexError (device lists: at the context's next check_index_error)."""
    what = "bag_pool"
    mode, denom = _pool_arg(what, pool)
    if out is H:
        raise ValueError(f"{what}: the output is the table that is pooled")
    if out.dim != H.dim:
        raise ValueError(f"{what}: output dim {out.dim} != table dim {H.dim}")
    if H.dim > 256:
        raise ValueError(f"{what}: dim {H.dim} above 256")
    pp, pi, B, n, dev, keep = _bags_arg(what, bags)
    row0 = 0
    if rows is not None:
        row0 = int(rows[0])
        if int(rows[1]) != B:
            raise ValueError(f"{what}: rows = {tuple(rows)} for {B} bags")
    if row0 < 0 or row0 + B > out.rows:
        raise ValueError(f"{what}: rows [{row0}, {row0 + B}) outside the {out.rows} output rows")
    H.ctx.after_torch(*keep[2:])
    H._sync_pending(); out._sync_pending()
    check(H.ctx._lib.orx_bag_pool(H.ctx._h, H._h, pp, pi, B, n, mode, denom, out._h, row0, _ffi.ORX_IDS_DEVICE if dev else 0))
    return out


class SeqRec:
    """A recommender without a user table: the user vector is pooled from the history table's rows of the items the user just
    interacted with,
        q = pool(H[history]);   s(q, i) = q . V[i] + b[i]
    (the depth-0 YouTube retrieval tower, FISM, item2vec).  H, V [items, D] are two Tables (never the same one), b [items, 1] or
    None.  pool: "mean", "sum" or ("fixed", denom).  `step` trains on one positive against N negatives per history
    (rt.multineg_step's objective with the user row replaced by q), `step_full` on the softmax over ALL items
    (rt.fullsoftmax_step's objective, the reference's); `user_table(bags)` gives the pooled rows as a Table that
    recommend_topk, rank_metrics_matrixfree, score_candidates and the samplers take with V and b as they stand, uid = the row
    number -- so a user never trained on is served from a history alone."""

    def __init__(self, H, V, b=None, pool="mean"):
        what = "SeqRec"
        _seqrec_check_tables(what, H, V, b)
        self._mode, self._denom = _pool_arg(what, pool)
        self.H, self.V, self.b, self.ctx, self.pool = H, V, b, H.ctx, pool
        self._Q = None

    def _args(self, what, loss, bags, pid, nid, weights, neg_offset):
        kind, N = _negatives_arg(what, loss, nid, exact=True)
        pp, pi, B, n, dev, kb = _bags_arg(what, bags)
        (ppid, pnid), (npid, nnid), _, keep = _id_lists(what, (pid, nid), dev)          # (on the side the bags are on)
        if npid != B or nnid != B * N:
            raise ValueError(f"{what}: {B} bags, {npid} positive ids and {nnid} negative ids for N = {N} "
                             "(one positive per bag, nid N times as long)")
        if B * (1 + N) >= 2 ** 31:
            raise ValueError(f"{what}: B * (1 + N) = {B * (1 + N)} must be below 2^31")
        pw, kw = _floats_arg(what, "weights", weights, dev, B, "the bags")
        po, ko = _floats_arg(what, "neg_offset", neg_offset, dev, nnid, "nid")
        self.ctx.after_torch(*kb, *keep, kw, ko)
        for t in (self.H, self.V, self.b):
            if t is not None:
                t._sync_pending()
        return kind, N, B, n, dev, (pp, pi, ppid, pnid, pw, po), (kb, keep, kw, ko)

    def step(self, opt, bags, pid, nid, loss="softmax", weights=None, neg_offset=None, l2_reg=0.0, train=None, want_loss=True):
        """One train step (orx_seqrec_step) on B histories: bag i against its positive pid[i] and the N negatives nid[i]
        ([B, N], N in 1 .. 64).  loss: "softmax" | "logsig"; weights [B]; neg_offset [B, N]; all live where the bags live.
        J = loss + l2_reg * l2_loss, the l2 term on the POOLED vector and the looked-up item rows.  train: None, or a subset of
        ("history", "item", "bias") -- every other table is read, never written.  -> (loss[1], l2[1]) as numpy float32, l2 the
        unscaled l2_loss, when want_loss, else None (ragged lists on the device: no host synchronisation).  Bad arguments raise
        ValueError before the library is called; a malformed device list or an id outside its table IndexError."""
        what = "SeqRec.step"
        mask = _mask_arg(what, train, _SEQ_ROLES, self.b is not None) or 0
        l2c = _coef_arg(what, "l2_reg", l2_reg)
        kind, N, B, n, dev, ptrs, keep = self._args(what, loss, bags, pid, nid, weights, neg_offset)
        out, lp, l2p = _loss_outputs(1, want_loss)
        check(self.ctx._lib.orx_seqrec_step(self.ctx._h, kind, opt._h, self.H._h, self.V._h, _bias_h(self.b), *ptrs, B, n, N,
                                            self._mode, self._denom, l2c, mask, _flags(dev), lp, l2p))
        _keep_tables(opt, (self.H, self.V, self.b))
        return out

    def loss(self, bags, pid, nid, loss="softmax", weights=None, neg_offset=None):
        """forward only: (loss, l2_loss) of one batch -- the step's own numbers bit for bit on the same tables; no table changes"""
        kind, N, B, n, dev, ptrs, keep = self._args("SeqRec.loss", loss, bags, pid, nid, weights, neg_offset)
        out, lp, l2p = _loss_outputs(1, True)
        check(self.ctx._lib.orx_seqrec_loss(self.ctx._h, kind, self.H._h, self.V._h, _bias_h(self.b), *ptrs, B, n, N, self._mode,
                                            self._denom, _flags(dev), lp, l2p))
        return _loss_pair(out)

    _FULL_STEP, _FULL_LOSS = ("orx_seqrec_full_step", "orx_seqrec_full_sets_step"), ("orx_seqrec_full_loss", "orx_seqrec_full_sets_loss")

    def _full_lists(self, bags):
        def lists(what):
            pp, pi, B, n, dev, kb = _bags_arg(what, bags)
            return pp, pi, B, n, dev, lambda: (), kb          # (no C arguments of the model's own)
        return lists

    def step_full(self, opt, bags, pid=None, weights=None, item_offset=None, scale=1.0, l2_reg=0.0, train=None, chunk_items=0,
                  chunk_samples=0, want_loss=True, labels=None, label_weights=None):
        """One train step on the softmax over ALL items (orx_seqrec_full_step): bag i's pooled vector against every row of the
        item table, the label pid[i] -- rt.fullsoftmax_step's objective with the user row replaced by q.  weights [B];
        item_offset [items], one float per item (-inf removes an item); both live where the bags live.  The history table goes
        `step`'s route, the item table and the bias take the optimizer's dense rule on every row.  train: None, or a subset
        of ("history", "item", "bias").  -> (loss[1], l2[1]) as numpy float32 when want_loss, else None.  Bad arguments raise
        ValueError before the library is called; a malformed device list or an id outside its table IndexError.
        labels= with pid=None (orx_seqrec_full_sets_step): a label SET per bag under the multinomial likelihood,
        l_i = T_i lse_i - sum_e t_e s_{i,j_e} -- Mult-DAE's objective.  labels is (ptr, items), ragged, no host synchronisation
        wherever it lives, or the padded pair (seq, seq_len); label_weights: t_e per entry (None: 1).  An empty set keeps the
        sample live with its l2 part alone; passing both pid and labels, or neither, raises."""
        what = "SeqRec.step_full"
        mask = _mask_arg(what, train, _SEQ_ROLES, self.b is not None) or 0
        l2c = _coef_arg(what, "l2_reg", l2_reg)
        return _full_step(what, self, self._FULL_STEP, self._full_lists(bags), (self.H, self.V, self.b), opt, (l2c,), mask, pid, weights,
                          item_offset, scale, chunk_items, chunk_samples, want_loss, labels, label_weights)

    def loss_full(self, bags, pid=None, weights=None, item_offset=None, scale=1.0, chunk_items=0, per_row=False, labels=None,
                  label_weights=None):
        """forward only: (loss, l2_loss) of one batch of step_full -- the step's own numbers bit for bit on the same tables; no
        table changes.  per_row=True: (loss, l2_loss, l) with l_i of every bag, a numpy float32 array [B].  labels= /
        label_weights= as step_full takes them"""
        return _full_loss("SeqRec.loss_full", self, self._FULL_LOSS, self._full_lists(bags), (self.H, self.V, self.b), pid, weights, item_offset,
                          scale, chunk_items, per_row, labels, label_weights)

    def user_table(self, bags, out=None):
        """-> a Table [B, D] of the pooled rows q_i of `bags` (out: a Table of that shape to write; None: one owned by this
        object, valid until the next call with another B).  With (V, b) it goes wherever a user table goes, uid = the row number."""
        what = "SeqRec.user_table"
        pp, pi, B, n, dev, keep = _bags_arg(what, bags)
        out = _owned_output(what, self, B, self.H.dim, out)
        return bag_pool(self.H, keep[2:], out, self.pool)           # (the ragged lists: a padded pair is converted once)

    def recommend(self, bags, k, excl=None):
        """the k best items for each history -> (item ids int32 [B, k], scores float32 [B, k]): recommend_topk("dot", ...) on
        user_table(bags); excl: a SparseMask or a dense bool mask [B, items] of items never returned (the history itself, say)"""
        Q = self.user_table(bags)
        return recommend_topk("dot", Q, self.V, self.b, np.arange(Q.rows, dtype=np.int32), k, excl=excl)


# ---- history-pooled recommender with a dense tower (orx_tower_step / orx_tower_loss / orx_tower_query) -------------------------------
_DEEP_ROLES = {**_SEQ_ROLES, "side": _ffi.ORX_TRAIN_SIDE, "tower": _ffi.ORX_TRAIN_TOWER}
_TOWER_LAYERS, _TOWER_SIDE, _TOWER_WIDTH = 4, 4, 256


def _handles(tables):
    """tables (None entries allowed) -> a C array of their handles"""
    return (c_void_p * max(len(tables), 1))(*[None if t is None else t._h for t in tables])


def tower_geometry(B, widths):
    """what the launcher of DeepSeqRec's tower does for B samples and the widths (in_0, out_0, ..., out_{L-1}): a dict of the rows
    per tile, the batch chunks of the backward, the tiles per chunk and the scratch bytes of a step with every table trained
    (beyond the lists' and the full softmax's).  No device is needed."""
    widths = [int(x) for x in widths]
    if not 2 <= len(widths) <= _TOWER_LAYERS + 1:
        raise ValueError(f"tower_geometry: {len(widths) - 1} layers (1 .. {_TOWER_LAYERS})")
    out = (c_int64 * 4)()
    check(_ffi.load().orx_tower_geometry(int(B), len(widths) - 1, (c_int32 * len(widths))(*widths), out))
    return dict(tile=int(out[0]), batch_chunks=int(out[1]), tiles_per_chunk=int(out[2]), scratch_bytes=int(out[3]))


class DeepSeqRec:
    """SeqRec with user-feature embeddings and hidden layers between the pool and the query (the reference's YouTubeRec):
        x0 = [ S_1[f_1] | ... | S_m[f_m] | pool(H[history]) ];   x_{l+1} = relu(x_l W_l + c_l);   q = x_L;   s(q, i) = q . V[i] + b[i]
    H [items, Dh], V [items, Dq], b [items, 1] or None.  layers: 1 .. 4 pairs (W_l [in_l, out_l], c_l [1, out_l] or None), or bare
    tables for layers without a bias; in_0 = sum d_j + Dh, out_{L-1} = Dq, every width in 1 .. 256.  side: 0 .. 4 Tables
    S_j [n_j, d_j], each indexed by one id list per call.  relu_last=False: the last layer is linear.  No table may be passed
    twice.  An EMPTY history pools to zeros and stays a live sample: in SeqRec its query is then 0 and only the item side takes a
    gradient; here the query comes from the side rows and the biases, and the layers and side rows take its gradient too."""

    def __init__(self, H, V, b, layers, side=(), pool="mean", relu_last=True):
        what = "DeepSeqRec"
        self._mode, self._denom = _pool_arg(what, pool)
        layers = [tuple(l) if isinstance(l, (tuple, list)) else (l, None) for l in layers]
        side = list(side)
        if not 1 <= len(layers) <= _TOWER_LAYERS:
            raise ValueError(f"{what}: {len(layers)} layers (1 .. {_TOWER_LAYERS})")
        if len(side) > _TOWER_SIDE:
            raise ValueError(f"{what}: {len(side)} side tables (0 .. {_TOWER_SIDE})")
        if any(len(l) != 2 or l[0] is None for l in layers):
            raise ValueError(f"{what}: a layer is (W, c) with c a Table or None")
        every = [H, V, b] + side + [t for l in layers for t in l]
        live = [t for t in every if t is not None]
        if len({id(t) for t in live}) != len(live):
            raise ValueError(f"{what}: a table is passed twice (tied tables are not offered)")
        if any(t.ctx is not H.ctx for t in live):
            raise ValueError(f"{what}: the tables live on different contexts")
        if H.rows != V.rows:
            raise ValueError(f"{what}: {H.rows} history rows for {V.rows} items")
        if b is not None and tuple(b.shape) != (V.rows, 1):
            raise ValueError(f"{what}: bias must be [{V.rows}, 1], got {list(b.shape)}")
        widths = [sum(s.dim for s in side) + H.dim]
        for l, (W, c) in enumerate(layers):
            if W.rows != widths[-1]:
                raise ValueError(f"{what}: layer {l} takes {W.rows} inputs where {widths[-1]} arrive (the widths do not chain)")
            if c is not None and tuple(c.shape) != (1, W.dim):
                raise ValueError(f"{what}: the bias of layer {l} is {list(c.shape)}, not [1, {W.dim}]")
            widths.append(W.dim)
        if widths[-1] != V.dim:
            raise ValueError(f"{what}: the last layer is {widths[-1]} wide, the item table has dim {V.dim}")
        bad = [w for w in widths + [s.dim for s in side] + [H.dim] if not 1 <= w <= _TOWER_WIDTH]
        if bad:
            raise ValueError(f"{what}: width {bad[0]} outside [1, {_TOWER_WIDTH}]")
        self.H, self.V, self.b, self.ctx, self.pool = H, V, b, H.ctx, pool
        self.layers, self.side, self.widths, self.relu_last = layers, side, widths, bool(relu_last)
        self._tables = live
        self._Q = None

    def _model_args(self, side_ptrs):
        """the side tables, their id pointers and the layers as the C arrays the three calls take"""
        m, L = len(self.side), len(self.layers)
        ids = (c_void_p * max(m, 1))(*side_ptrs)
        arrays = (_handles(self.side), ids, _handles([W for W, _ in self.layers]), _handles([c for _, c in self.layers]))
        return (m, arrays[0], arrays[1], L, arrays[2], arrays[3], int(self.relu_last)), arrays

    def _lists(self, what, bags, side_ids):
        pp, pi, B, n, dev, kb = _bags_arg(what, bags)
        side_ids = tuple(side_ids)
        if len(side_ids) != len(self.side):
            raise ValueError(f"{what}: {len(side_ids)} side id lists for {len(self.side)} side tables")
        ps, ns, _, ks = _id_lists(what, side_ids, dev)                  # (on the side the bags are on)
        if any(x != B for x in ns):
            raise ValueError(f"{what}: {B} bags and side id lists of {ns} ids (one id per bag and side table)")
        return pp, pi, B, n, dev, ps, (kb, ks)

    _FULL_STEP, _FULL_LOSS = ("orx_tower_step", "orx_tower_sets_step"), ("orx_tower_loss", "orx_tower_sets_loss")

    def _full_lists(self, bags, side_ids):
        def lists(what):
            pp, pi, B, n, dev, ps, keep = self._lists(what, bags, side_ids)
            return pp, pi, B, n, dev, lambda: self._model_args(ps)[0], keep          # (the C arrays live as long as the tuple that holds them)
        return lists

    def step_full(self, opt, bags, pid=None, side_ids=(), weights=None, item_offset=None, scale=1.0, l2_reg=0.0, l2_mlp=0.0, train=None,
                  chunk_items=0, chunk_samples=0, want_loss=True, labels=None, label_weights=None):
        """One train step on the softmax over ALL items (orx_tower_step): SeqRec.step_full's objective with the query computed by
        the tower.  side_ids: one id list [B] per side table, where the bags live.  J = loss + l2_reg * l2_loss + l2_mlp * 1/2
        sum_l (|W_l|^2 + |c_l|^2), l2_loss = 1/2 (sum |x0_i|^2 + sum |V[pid_i]|^2) on the embedding outputs.  The history table
        goes SeqRec's sorted route, a side table takes the sparse rule on its id list, V, b and every W_l, c_l the optimizer's
        dense rule.  train: None, or a subset of ("history", "item", "bias", "side", "tower").  -> (loss[1], l2[1]) as numpy
        float32, l2 the unscaled l2_loss, when want_loss, else None.  Bad arguments raise ValueError before the library is
        called; a malformed device list or an id outside its table IndexError.  labels= / label_weights= with pid=None
        (orx_tower_sets_step): a label set per bag, as SeqRec.step_full takes them -- Mult-DAE with hidden layers."""
        what = "DeepSeqRec.step_full"
        mask = _mask_arg(what, train, _DEEP_ROLES, self.b is not None) or 0
        if mask & _ffi.ORX_TRAIN_SIDE and not self.side:
            raise ValueError(f'{what}: train: "side" named, but the model has no side table')
        l2c, l2m = _coef_arg(what, "l2_reg", l2_reg), _coef_arg(what, "l2_mlp", l2_mlp)
        return _full_step(what, self, self._FULL_STEP, self._full_lists(bags, side_ids), self._tables, opt, (l2c, l2m), mask, pid, weights,
                          item_offset, scale, chunk_items, chunk_samples, want_loss, labels, label_weights)

    def loss_full(self, bags, pid=None, side_ids=(), weights=None, item_offset=None, scale=1.0, chunk_items=0, per_row=False,
                  labels=None, label_weights=None):
        """forward only: (loss, l2_loss) of one batch of step_full -- the step's own numbers bit for bit on the same tables; no
        table changes.  per_row=True: (loss, l2_loss, l) with l_i of every bag, a numpy float32 array [B].  labels= /
        label_weights= as step_full takes them"""
        return _full_loss("DeepSeqRec.loss_full", self, self._FULL_LOSS, self._full_lists(bags, side_ids), self._tables, pid, weights,
                          item_offset, scale, chunk_items, per_row, labels, label_weights)

    def user_table(self, bags, side_ids=(), out=None):
        """-> a Table [B, Dq] of the queries q_i (orx_tower_query) -- the rows the step scores with, bit for bit, and a row's bits
        do not depend on the batch around it.  out: a Table of that shape to write; None: one owned by this object, valid until
        the next call with another B.  With (V, b) it goes wherever a user table goes, uid = the row number."""
        what = "DeepSeqRec.user_table"
        pp, pi, B, n, dev, ps, keep = self._lists(what, bags, side_ids)
        out = _owned_output(what, self, B, self.V.dim, out, "bags and queries")
        if any(out is t for t in self._tables):
            raise ValueError(f"{what}: the output is one of the model's tables")
        self.ctx.after_torch(*keep[0], *keep[1])
        for t in self._tables:
            t._sync_pending()
        out._sync_pending()
        model, arrays = self._model_args(ps)
        check(self.ctx._lib.orx_tower_query(self.ctx._h, self.H._h, *model, pp, pi, B, n, self._mode, self._denom, out._h, 0, _flags(dev)))
        return out

    def recommend(self, bags, side_ids, k, excl=None):
        """the k best items for each history -> (item ids int32 [B, k], scores float32 [B, k]): recommend_topk("dot", ...) on
        user_table(bags, side_ids); excl: a SparseMask or a dense bool mask [B, items] of items never returned"""
        Q = self.user_table(bags, side_ids)
        return recommend_topk("dot", Q, self.V, self.b, np.arange(Q.rows, dtype=np.int32), k, excl=excl)
