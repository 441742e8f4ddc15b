"""A recording stand-in for everything openrec_amd.runtime's train-step and forward-loss calls touch: a library whose orx_*
functions write down (name, args) and return 0, a context that writes down what after_torch was given, tables and an optimizer
with handles only, and fake device tensors.  No library and no device is needed.  `run` makes one call of one of the twenty
entry points on a fresh set of these and returns what happened; tests/test_runtime_args_cpu.py and scripts/runtime_args_ab.py are
built on it."""
import numpy as np

K, B, STRIDE, N, D = 2, 4, 5, 3, 8          # the smallest shape that tells the cases apart:
NEED = (K - 1) * STRIDE + B                 # 9 ids a list needs
USERS, ITEMS, FD, DC = 20, 30, 6, 3

ENTRIES = ("pairwise_step", "pairwise_loss", "pointwise_step", "pointwise_loss", "multineg_step", "multineg_loss", "inbatch_step",
           "inbatch_loss", "LightGCN.step", "LightGCN.loss", "VBPR.step", "VBPR.loss", "SeqRec.step", "SeqRec.loss", "fullsoftmax_step", "fullsoftmax_loss",
           "SeqRec.step_full", "SeqRec.loss_full", "DeepSeqRec.step_full", "DeepSeqRec.loss_full")
FULL = ENTRIES[14:]                         # the calls on the softmax over all items: item_offset is one float per ITEM
STEPS = tuple(e for e in ENTRIES if "step" in e.split(".")[-1])
SIDE, HID = ((5, 2), (7, 3)), 6             # DeepSeqRec: two side tables [rows, dim]; W0 [2 + 3 + D, HID] with a bias, W1 [HID, D] without one


class NoDevice:
    """stands where a table, an optimizer or a context would: any use of it is a device call the check should have come before"""

    def __getattr__(self, name):
        raise AssertionError(f"the runtime reached for .{name} before it refused the call")


class FakeDeviceTensor:
    """what the runtime asks of a torch device tensor, int32 or float32"""
    is_cuda = True
    _next = 0x7f0000000000

    def __init__(self, shape, dtype="int32"):
        self.shape = tuple(np.atleast_1d(shape).tolist())
        self.dtype = "torch." + dtype
        FakeDeviceTensor._next += 0x100000
        self._ptr, self._n = FakeDeviceTensor._next, int(np.prod(self.shape))

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return self._n

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return True


class RecordingLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("orx_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


class RecordingContext:
    _h, device = "h:ctx", 0

    def __init__(self):
        self._lib = RecordingLib()
        self.ordered = []          # one tuple per after_torch call

    def after_torch(self, *tensors):
        self.ordered.append(tensors)

    def check_index_error(self):
        self._lib.calls.append(("check_index_error", ()))


class StandinTable:
    def __init__(self, ctx, name, rows, dim, handle=None):          # handle: an integer one, for a table that travels in a C array
        self.ctx, self._h, self.rows, self.dim, self.shape, self.flushes = ctx, handle or "h:" + name, rows, dim, (rows, dim), 0
        self.name = name

    def _sync_pending(self):
        self.flushes += 1


class StandinOptimizer:
    _h = "h:opt"

    def __init__(self):
        self._tables = []


class World:
    """one context with its tables, optimizer and the three model objects"""

    def __init__(self, rt, bias=True):
        self.rt, self.ctx, self.opt = rt, RecordingContext(), StandinOptimizer()
        T = lambda name, rows, dim: StandinTable(self.ctx, name, rows, dim)
        self.U, self.V, self.b, self.w = T("U", USERS, D), T("V", ITEMS, D), (T("b", ITEMS, 1) if bias else None), T("w", D, 1)
        self.H, self.E, self.Uv = T("H", ITEMS, D), T("E", FD, DC), T("Uv", USERS, D + DC)
        A = lambda i, name, rows, dim: StandinTable(self.ctx, name, rows, dim, 0x1000 + i)
        self.S = [A(j, f"S{j}", rows, dim) for j, (rows, dim) in enumerate(SIDE)]
        self.W0, self.c0, self.W1 = A(4, "W0", sum(d for _, d in SIDE) + D, HID), A(5, "c0", 1, HID), A(6, "W1", HID, D)

    @property
    def calls(self):
        return self.ctx._lib.calls

    def tables(self):
        return [t for t in (self.U, self.V, self.b, self.w, self.H, self.E, self.Uv, *self.S, self.W0, self.c0, self.W1) if t is not None]

    def lightgcn(self):
        m = self.rt.LightGCN.__new__(self.rt.LightGCN)
        m.U, m.V, m.ctx, m._h, m._fresh = self.U, self.V, self.ctx, "h:lightgcn", True
        return m

    def vbpr(self):
        f = object.__new__(self.rt.ItemFeatures)
        f.ctx, f.rows, f.dim, f._ptr = self.ctx, ITEMS, FD, 0x7e0000000000
        return self.rt.VBPR(self.Uv, self.V, self.b, self.E, f)

    def seqrec(self):
        return self.rt.SeqRec(self.H, self.V, self.b, pool=("fixed", 2.0))

    def deepseqrec(self):
        return self.rt.DeepSeqRec(self.H, self.V, self.b, [(self.W0, self.c0), self.W1], side=self.S, pool=("fixed", 2.0), relu_last=False)


def make_list(shape, dev, dtype="int32", fill=1):
    if dev:
        return FakeDeviceTensor(shape, dtype)
    return np.full(shape, fill, np.dtype(dtype))


# the lists of each entry point: name -> (dtype, length in units of the id count n; "N": n * N shaped [n, N]); optional ones last
_LISTS = {
    "pairwise": (("uid", "int32", 1), ("pid", "int32", 1), ("nid", "int32", 1), ("weights", "float32", 1)),
    "pointwise": (("uid", "int32", 1), ("iid", "int32", 1), ("label", "float32", 1)),
    "multineg": (("uid", "int32", 1), ("pid", "int32", 1), ("nid", "int32", "N"), ("weights", "float32", 1), ("neg_offset", "float32", "N")),
    "inbatch": (("uid", "int32", 1), ("pid", "int32", 1), ("weights", "float32", 1), ("item_offset", "float32", 1)),
    "SeqRec": (("ptr", "int32", "ptr"), ("items", "int32", "items"), ("pid", "int32", 1), ("nid", "int32", "N"), ("weights", "float32", 1),
               ("neg_offset", "float32", "N")),
}
_LISTS["LightGCN"] = _LISTS["pairwise"][:3]
_LISTS["VBPR"] = _LISTS["pairwise"]
# the full softmax: item_offset has ITEMS entries; a bag form takes pid or -- labels="ragged" / "padded" -- a label set per bag
_LABELS = (("lab_ptr", "int32", "ptr"), ("lab_items", "int32", "items"), ("lab_seq", "int32", "L"), ("lab_len", "int32", 1),
           ("label_weights", "float32", "items"))
_LISTS["fullsoftmax"] = (("uid", "int32", 1), ("pid", "int32", 1), ("weights", "float32", 1), ("item_offset", "float32", "I"))
_LISTS["SeqRec.full"] = (("ptr", "int32", "ptr"), ("items", "int32", "items"), ("pid", "int32", 1), *_LABELS, ("weights", "float32", 1),
                         ("item_offset", "float32", "I"))
_LISTS["DeepSeqRec.full"] = (*_LISTS["SeqRec.full"][:2], ("f0", "int32", 1), ("f1", "int32", 1), *_LISTS["SeqRec.full"][2:])
OPTIONAL = ("weights", "neg_offset", "item_offset")
LABEL_LISTS = {None: ("pid",), "ragged": ("lab_ptr", "lab_items"), "padded": ("lab_seq", "lab_len")}


def family(entry):
    if entry.endswith("_full"):
        return entry.split(".")[0] + ".full"
    return entry.split(".")[0].rsplit("_", 1)[0]


def make_lists(entry, dev, n, optional=(), over=None, labels=None):
    """the lists of one call: every required one and the `optional` ones named, n ids each on the side `dev`; over:
    {name: dict(dev=, shape=) or an object to pass as it is} for the lists that break the rule; labels: None (pid), "ragged"
    or "padded" (two label items per bag; padded: the pair [n, 3], [n]), with "label_weights" among `optional` or not"""
    out = {}
    for name, dtype, unit in _LISTS[family(entry)]:
        if name in OPTIONAL and name not in optional and name not in (over or {}):
            continue
        if name in ("pid",) + tuple(x[0] for x in _LABELS) and family(entry).endswith(".full"):
            if name not in LABEL_LISTS[labels] + (("label_weights",) if labels and "label_weights" in optional else ()) and name not in (over or {}):
                continue
        shape = {1: (n,), "N": (n, N), "ptr": (n + 1,), "items": (2 * n,), "I": (ITEMS,), "L": (n, 3)}[unit]
        if name == "label_weights" and labels == "padded":
            shape = (n, 3)
        spec = (over or {}).get(name, {})
        if not isinstance(spec, dict):
            out[name] = spec
            continue
        x = make_list(spec.get("shape", shape), spec.get("dev", dev), dtype)
        if name in ("ptr", "lab_ptr") and not spec.get("dev", dev):
            x[:] = 2 * np.arange(x.size)          # n bags of two items each
        if name == "lab_len" and not spec.get("dev", dev):
            x[:] = 2
        out[name] = x
    return out


def call(w, entry, L, kw):
    """the entry point called the way its signature reads, on the world's tables"""
    rt, kw = w.rt, dict(kw)
    if entry == "pairwise_step":
        return rt.pairwise_step(kw.pop("model", "bpr"), w.opt, w.U, w.V, w.b, L["uid"], L["pid"], L["nid"], weights=L.get("weights"), **kw)
    if entry == "pairwise_loss":
        return rt.pairwise_loss(kw.pop("model", "bpr"), w.U, w.V, w.b, L["uid"], L["pid"], L["nid"], weights=L.get("weights"), **kw)
    if entry == "pointwise_step":
        return rt.pointwise_step(kw.pop("model", "wrmf"), w.opt, w.U, w.V, w.b, kw.pop("w", None), L["uid"], L["iid"], L["label"], **kw)
    if entry == "pointwise_loss":
        return rt.pointwise_loss(kw.pop("model", "wrmf"), w.U, w.V, w.b, kw.pop("w", None), L["uid"], L["iid"], L["label"], **kw)
    if entry == "multineg_step":
        return rt.multineg_step(kw.pop("loss", "softmax"), w.opt, w.U, w.V, w.b, L["uid"], L["pid"], L["nid"], weights=L.get("weights"),
                                neg_offset=L.get("neg_offset"), **kw)
    if entry == "multineg_loss":
        return rt.multineg_loss(kw.pop("loss", "softmax"), w.U, w.V, w.b, L["uid"], L["pid"], L["nid"], weights=L.get("weights"),
                                neg_offset=L.get("neg_offset"), **kw)
    if entry == "inbatch_step":
        return rt.inbatch_step(w.opt, w.U, w.V, w.b, L["uid"], L["pid"], weights=L.get("weights"), item_offset=L.get("item_offset"), **kw)
    if entry == "inbatch_loss":
        return rt.inbatch_loss(w.U, w.V, w.b, L["uid"], L["pid"], weights=L.get("weights"), item_offset=L.get("item_offset"), **kw)
    if entry == "LightGCN.step":
        return w.lightgcn().step(w.opt, L["uid"], L["pid"], L["nid"], **kw)
    if entry == "LightGCN.loss":
        return w.lightgcn().loss(L["uid"], L["pid"], L["nid"], **kw)
    if entry == "VBPR.step":
        return w.vbpr().step(w.opt, L["uid"], L["pid"], L["nid"], weights=L.get("weights"), **kw)
    if entry == "VBPR.loss":
        return w.vbpr().loss(L["uid"], L["pid"], L["nid"], weights=L.get("weights"), **kw)
    if entry == "SeqRec.step":
        return w.seqrec().step(w.opt, (L["ptr"], L["items"]), L["pid"], L["nid"], weights=L.get("weights"), neg_offset=L.get("neg_offset"), **kw)
    if entry == "SeqRec.loss":
        return w.seqrec().loss((L["ptr"], L["items"]), L["pid"], L["nid"], weights=L.get("weights"), neg_offset=L.get("neg_offset"), **kw)
    if entry in ("fullsoftmax_step", "fullsoftmax_loss"):
        head = (w.opt,) if entry.endswith("step") else ()
        return getattr(rt, entry)(*head, w.U, w.V, w.b, L["uid"], L["pid"], weights=L.get("weights"), item_offset=L.get("item_offset"), **kw)
    if entry in FULL:
        model = w.seqrec() if entry.startswith("SeqRec") else w.deepseqrec()
        head = (w.opt,) if entry.endswith("step_full") else ()
        if "lab_ptr" in L or "lab_seq" in L:
            kw.update(labels=(L["lab_ptr"], L["lab_items"]) if "lab_ptr" in L else (L["lab_seq"], L["lab_len"]))
        kw.update(label_weights=L.get("label_weights"))
        if entry.startswith("Deep"):
            kw.setdefault("side_ids", (L["f0"], L["f1"]))
        return getattr(model, entry.split(".")[1])(*head, (L["ptr"], L["items"]), L.get("pid"), weights=L.get("weights"),
                                                   item_offset=L.get("item_offset"), **kw)
    raise KeyError(entry)


class Outcome:
    """what one call did: .result or .error, .calls (the library's record), .ordered (after_torch's), .lists (name -> object),
    .world"""

    def pointer_of(self, name):
        x = self.lists[name]
        return x.data_ptr() if isinstance(x, FakeDeviceTensor) else x.ctypes.data

    def ordered_lists(self):
        """the names of the device lists that after_torch was handed, over all its calls"""
        return {k for k, x in self.lists.items() if isinstance(x, FakeDeviceTensor) and any(x is t for group in self.ordered for t in group)}

    def only_call(self):
        calls = [c for c in self.calls if c[0] != "check_index_error"]
        assert len(calls) == 1, self.calls
        return calls[0]


def run(rt, entry, dev=False, n=NEED, optional=(), over=None, bias=True, labels=None, **kw):
    """one call of `entry` on a fresh world; an exception is caught and kept"""
    o = Outcome()
    o.world = World(rt, bias)
    o.lists = make_lists(entry, dev, n, optional, over, labels)
    o.result = o.error = None
    try:
        o.result = call(o.world, entry, o.lists, kw)
    except Exception as e:          # (whatever it is: the caller looks at the type)
        o.error = e
    o.calls, o.ordered = o.world.calls, o.world.ctx.ordered
    return o


def describe(o):
    """one line for a dump: the exception's type, or the C call with every pointer named after the list it came from"""
    if o.error is not None:
        return type(o.error).__name__
    where = {o.pointer_of(k): k for k, x in o.lists.items() if isinstance(x, (FakeDeviceTensor, np.ndarray))}
    named = {**where, **{t._h: t.name for t in o.world.tables() if isinstance(t._h, int)}}
    out = []
    for fn, args in o.calls:
        shown = []
        for a in args:
            if hasattr(a, "_length_"):          # a C array of handles or pointers
                shown.append("[" + ", ".join(named.get(v, repr(v)) for v in a) + "]")
            elif isinstance(a, (int, np.integer)) and not isinstance(a, bool) and int(a) in where:
                shown.append(where[int(a)] + "+0")
            elif isinstance(a, (int, np.integer)) and int(a) >= 1 << 32:
                base = [k for p, k in where.items() if p < int(a) < p + 4 * max(o.lists[k].size if isinstance(o.lists[k], np.ndarray) else o.lists[k].numel(), 1)]
                shown.append(f"{base[0]}+{int(a) - o.pointer_of(base[0])}" if base else "ptr")
            elif isinstance(a, (int, float, str, type(None), np.integer, np.floating)):
                shown.append(repr(a if not isinstance(a, (np.integer, np.floating)) else a.item()))
            else:
                shown.append(type(a).__name__)
        out.append(f"{fn}({', '.join(shown)})")
    flushed = "".join(t.name for t in o.world.tables() if t.flushes)
    ordered = sorted(o.ordered_lists())
    res ="None" if o.result is None else "floats" if isinstance(o.result[0], float) else f"arrays{[len(r) for r in o.result]}"
    return "; ".join(out) + f" | flushed: {flushed or '-'} | after_torch: {ordered} | -> {res}"
