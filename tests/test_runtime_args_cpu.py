"""The argument layer of the runtime's train-step and forward-loss calls, on the recording stand-in of
tests/runtime_standin.py: what reaches the library for a good call, and that a bad one is a ValueError naming the call before
anything reaches it.  No library and no device."""
import math

import numpy as np
import pytest

import runtime_standin as si
from runtime_standin import B, ENTRIES, FD, FULL, ITEMS, K, N, NEED, STEPS, STRIDE, run

from openrec_amd import _ffi
from openrec_amd import runtime as rt

OUT, REF = object(), object()          # an output pointer the wrapper made itself; a ctypes byref
DEV, HOG, NOL2, CENSOR, SIG, HITS = (_ffi.ORX_IDS_DEVICE, _ffi.ORX_HOGWILD, _ffi.ORX_NO_L2, _ffi.ORX_CENSOR, _ffi.ORX_POINT_SIGMOID,
                                      _ffi.ORX_IB_MASK_HITS)
SHAPE = dict(K=K, B=B, id_stride=STRIDE)
KSTEP = ("pairwise_step", "pointwise_step", "multineg_step", "inbatch_step", "VBPR.step")          # the calls that take K, B, id_stride
OVERLAP = ("pairwise_step", "pointwise_step")          # their C side takes any id_stride; the others' refuses one below B
FPTR =0x7e0000000000          # the stand-in features' device pointer


def shape_kw(entry):
    return SHAPE if entry in KSTEP else {}


def assert_call(o, fn, want):
    assert o.error is None, repr(o.error)
    name, args = o.only_call()
    assert name == fn and len(args) == len(want), (name, args)
    for i, (a, w) in enumerate(zip(args, want)):
        if w is OUT:
            assert isinstance(a, int) and a > 0, (fn, i, a)
        elif w is REF:
            assert type(a).__name__ == "CArgObject", (fn, i, a)
        elif isinstance(w, str) and w.startswith("@"):
            assert a == o.pointer_of(w[1:]), (fn, i, a, w)
        elif isinstance(w, list):          # a C array: handles, or "@list" pointers
            assert list(a) == [o.pointer_of(x[1:]) if isinstance(x, str) else x for x in w], (fn, i, list(a), w)
        else:
            assert a == w and (a is None) == (w is None) and isinstance(a, float) == isinstance(w, float), (fn, i, a, w)


def expected(entry, f):
    """the C function and its arguments for the plain call of `entry` with every optional list present (where it takes any),
    K = 2, B = 4, id_stride = 5 over 9 ids (a forward-only call: B = 9); f: ORX_IDS_DEVICE or 0"""
    tri, outs = ("@uid", "@pid", "@nid"), (OUT, OUT)
    if entry in FULL:
        return expected_full(entry, f)
    return {
        "pairwise_step": ("orx_pairwise_step_weighted", ("h:ctx", _ffi.ORX_BPR, "h:opt", "h:U", "h:V", "h:b", *tri, "@weights", 2, 4, 5, 0.5, 1.0,
                                                        f, 0, *outs)),
        "pairwise_loss": ("orx_pairwise_loss_weighted", ("h:ctx", _ffi.ORX_BPR, "h:U", "h:V", "h:b", *tri, "@weights", 9, 0.5, f, *outs)),
        "pointwise_step": ("orx_pointwise_step", ("h:ctx", _ffi.ORX_WRMF, "h:opt", "h:U", "h:V", "h:b", None, "@uid", "@iid", "@label", 2, 4, 5,
                                                  1.0, 1.0, f, *outs)),
        "pointwise_loss": ("orx_pointwise_loss", ("h:ctx", _ffi.ORX_WRMF, "h:U", "h:V", "h:b", None, "@uid", "@iid", "@label", 9, 1.0, 1.0, f, *outs)),
        "multineg_step": ("orx_multineg_step", ("h:ctx", _ffi.ORX_MN_SOFTMAX, "h:opt", "h:U", "h:V", "h:b", *tri, "@weights", "@neg_offset",
                                                2, 4, 3, 5, 1.0, f, *outs)),
        "multineg_loss": ("orx_multineg_loss", ("h:ctx", _ffi.ORX_MN_SOFTMAX, "h:U", "h:V", "h:b", *tri, "@weights", "@neg_offset", 9, 3, f, *outs)),
        "inbatch_step": ("orx_inbatch_step", ("h:ctx", "h:opt", "h:U", "h:V", "h:b", "@uid", "@pid", "@weights", "@item_offset", 2, 4, 5, 1.0, 1.0, 0,
                                              f | HITS, *outs)),
        "inbatch_loss": ("orx_inbatch_loss", ("h:ctx", "h:U", "h:V", "h:b", "@uid", "@pid", "@weights", "@item_offset", 9, 1.0, 0, f | HITS, *outs, None)),
        "LightGCN.step": ("orx_lightgcn_step", ("h:lightgcn", "h:opt", *tri, 9, 0.0, 0, f, REF, REF)),
        "LightGCN.loss": ("orx_lightgcn_loss", ("h:lightgcn", *tri, 9, 0.0, f, REF, REF)),
        "VBPR.step": ("orx_vbpr_step", ("h:ctx", "h:opt", "h:Uv", "h:V", "h:b", "h:E", FPTR, ITEMS, FD, *tri, "@weights", 2, 4, 5, 0.0, 0.0, 0, 0, f, *outs)),
        "VBPR.loss": ("orx_vbpr_loss", ("h:ctx", "h:Uv", "h:V", "h:b", "h:E", FPTR, ITEMS, FD, *tri, "@weights", 9, f, *outs)),
        "SeqRec.step": ("orx_seqrec_step", ("h:ctx", _ffi.ORX_MN_SOFTMAX, "h:opt", "h:H", "h:V", "h:b", "@ptr", "@items", "@pid", "@nid", "@weights",
                                            "@neg_offset", 9, 18, 3, _ffi.ORX_BAG_FIXED, 2.0, 0.0, 0, f, *outs)),
        "SeqRec.loss": ("orx_seqrec_loss", ("h:ctx", _ffi.ORX_MN_SOFTMAX, "h:H", "h:V", "h:b", "@ptr", "@items", "@pid", "@nid", "@weights",
                                            "@neg_offset", 9, 18, 3, _ffi.ORX_BAG_FIXED, 2.0, f, *outs)),
    }[entry]


FIXED = _ffi.ORX_BAG_FIXED
TOWER = (2, [0x1000, 0x1001], ["@f0", "@f1"], 2, [0x1004, 0x1006], [0x1005, None], 0)          # the stand-in's DeepSeqRec as the C calls take it


def expected_full(entry, f, labels=None, label_weights=True, optional=True, bias=True, l2=(0.0, 0.0), chunks=(0, 0), mask=0, scale=1.0, outs=(OUT, OUT),
                  rows=None):
    """the same for the six calls on the softmax over all items; labels: None (pid), or "ragged" (the label lists reach the
    library as they came); the rest: what the call was given beyond the defaults"""
    b, wt, off = "h:b" if bias else None, "@weights" if optional else None, "@item_offset" if optional else None
    step = "step" in entry
    if entry.startswith("fullsoftmax"):
        tail = (9, scale, l2[0], *chunks, mask, f, *outs) if step else (9, scale, chunks[0], f, OUT, OUT, rows)
        return "orx_" + entry, ("h:ctx", *(("h:opt",) if step else ()), "h:U", "h:V", b, "@uid", "@pid", wt, off, *tail)
    deep = entry.startswith("Deep")
    lab = ("@pid",) if labels is None else ("@lab_ptr", "@lab_items", "@label_weights" if label_weights else None, 18)
    coef = (l2 if deep else l2[:1])
    tail = (9, 18, FIXED, 2.0, scale, *coef, *chunks, mask, f, *outs) if step else (9, 18, FIXED, 2.0, scale, chunks[0], f, OUT, OUT, rows)
    name = ("orx_tower" if deep else "orx_seqrec_full") + ("_sets" if labels else "") + ("_step" if step else "_loss")
    return name, ("h:ctx", *(("h:opt",) if step else ()), "h:H", "h:V", b, *(TOWER if deep else ()), "@ptr", "@items", *lab, wt, off, *tail)


DEEP_TABLES = "S0S1W0c0W1"
FLUSHED = {"LightGCN": "UV", "VBPR": "VbEUv", "SeqRec": "VbH", "SeqRec.full": "VbH",          # the tables a family flushes, in World.tables() order
           "DeepSeqRec.full": "VbH" + DEEP_TABLES}


def flushed(o):
    return "".join(t.name for t in o.world.tables() if t.flushes)


# ---- 1. the C call ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_the_c_call_of_every_entry_point(entry, dev):
    o = run(rt, entry, dev, optional=si.OPTIONAL, **shape_kw(entry))
    assert_call(o, *expected(entry, DEV if dev else 0))
    # the library's stream is ordered behind torch for every device list, and the flushes are the family's own
    assert o.ordered_lists() == (set(o.lists) if dev else set())
    assert flushed(o) == FLUSHED.get(si.family(entry), "")
    if "loss" in entry.split(".")[-1] or entry == "LightGCN.step":
        assert isinstance(o.result, tuple) and len(o.result) == 2 and all(isinstance(x, float) for x in o.result)
    else:
        k = K if entry in KSTEP else 1
        assert all(isinstance(x, np.ndarray) and x.dtype == np.float32 and x.shape == (k,) for x in o.result) and len(o.result) == 2
    if dev and entry.startswith("LightGCN"):
        assert o.calls[-1] == ("check_index_error", ())          # (stays: device ids report a bad id at the next check)


def _tail(o, k):
    return o.only_call()[1][-k:]


@pytest.mark.parametrize("dev,f", [(False, 0), (True, DEV)], ids=["host", "device"])
def test_pairwise_step_routing(dev, f):
    head = ("h:ctx", _ffi.ORX_BPR, "h:opt", "h:U", "h:V", "h:b", "@uid", "@pid", "@nid")
    go = lambda **kw: run(rt, "pairwise_step", dev, **SHAPE, **kw)
    assert_call(go(), "orx_pairwise_step", (*head, 2, 4, 5, 0.5, f, OUT, OUT))
    assert_call(go(model="ucml", margin=0.25, hogwild=True, censor=True, no_l2=True, want_loss=False), "orx_pairwise_step",
                (*head[:1], _ffi.ORX_UCML, *head[2:], 2, 4, 5, 0.25, f | HOG | NOL2 | CENSOR, None, None))
    assert_call(go(train=("user", "bias")), "orx_pairwise_step_subset", (*head, 2, 4, 5, 0.5, f, 5, OUT, OUT))
    assert_call(go(train="item", no_l2=True), "orx_pairwise_step_subset", (*head, 2, 4, 5, 0.5, f | NOL2, 2, OUT, OUT))
    assert_call(go(optional=("weights",)), "orx_pairwise_step_weighted", (*head, "@weights", 2, 4, 5, 0.5, 1.0, f, 0, OUT, OUT))
    assert_call(go(l2_reg=0.25, train=("item",)), "orx_pairwise_step_weighted", (*head, None, 2, 4, 5, 0.5, 0.25, f, 2, OUT, OUT))
    # no_l2 with weights is the coefficient 0 and no flag; with an l2_reg of the caller's own it is refused (below)
    assert_call(go(optional=("weights",), no_l2=True, hogwild=True), "orx_pairwise_step_weighted",
                (*head, "@weights", 2, 4, 5, 0.5, 0.0, f | HOG, 0, OUT, OUT))
    assert_call(go(bias=False), "orx_pairwise_step", (*head[:5], None, *head[6:], 2, 4, 5, 0.5, f, OUT, OUT))
    assert_call(run(rt, "pairwise_loss", dev), "orx_pairwise_loss", ("h:ctx", _ffi.ORX_BPR, "h:U", "h:V", "h:b", *head[6:], 9, 0.5, f, OUT, OUT))
    assert_call(run(rt, "pairwise_loss", dev, bias=False, model="ucml", margin=1.5), "orx_pairwise_loss",
                ("h:ctx", _ffi.ORX_UCML, "h:U", "h:V", None, *head[6:], 9, 1.5, f, OUT, OUT))


@pytest.mark.parametrize("dev,f", [(False, 0), (True, DEV)], ids=["host", "device"])
def test_pointwise_step_routing(dev, f):
    head = ("h:ctx", _ffi.ORX_WRMF, "h:opt", "h:U", "h:V", "h:b", None, "@uid", "@iid", "@label", 2, 4, 5)
    go = lambda **kw: run(rt, "pointwise_step", dev, **SHAPE, **kw)
    assert_call(go(a=2.0, b_w=0.5, sigmoid=True, hogwild=True, no_l2=True, want_loss=False), "orx_pointwise_step",
                (*head, 2.0, 0.5, f | HOG | NOL2 | SIG, None, None))
    o = go(model="gmf", w=si.StandinTable(None, "w", 8, 1))
    assert_call(o, "orx_pointwise_step", (head[0], _ffi.ORX_GMF, *head[2:6], "h:w", *head[7:], 1.0, 1.0, f, OUT, OUT))
    assert_call(go(train=("user", "item")), "orx_pointwise_step_subset", (*head, 1.0, 1.0, f, 3, OUT, OUT))
    assert_call(go(l2_reg=0.01), "orx_pointwise_step_l2reg", (*head, 1.0, 1.0, 0.01, f, 0, OUT, OUT))
    assert_call(go(l2_reg=0.0, train="bias", sigmoid=True), "orx_pointwise_step_l2reg", (*head, 1.0, 1.0, 0.0, f | SIG, 4, OUT, OUT))
    assert_call(run(rt, "pointwise_loss", dev, sigmoid=True, a=3.0), "orx_pointwise_loss",
                ("h:ctx", _ffi.ORX_WRMF, "h:U", "h:V", "h:b", None, "@uid", "@iid", "@label", 9, 3.0, 1.0, f | SIG, OUT, OUT))


def test_the_other_families_options():
    """no_l2 with and without an l2_reg, bias=None, no optional list, the masks and the coefficients"""
    o = run(rt, "multineg_step", bias=False, loss="logsig", no_l2=True, want_loss=False, **SHAPE)
    assert o.only_call()[1][1] == _ffi.ORX_MN_LOGSIG and o.only_call()[1][5] is None and o.result is None
    assert o.only_call()[1][9:] == (None, None, 2, 4, 3, 5, 0.0, 0, None, None)
    assert _tail(run(rt, "multineg_step", l2_reg=0.5, **SHAPE), 4)[:2] == (0.5, 0)
    assert _tail(run(rt, "multineg_step", l2_reg=0.0, no_l2=True, **SHAPE), 4)[:2] == (0.0, 0)
    assert _tail(run(rt, "inbatch_step", True, no_l2=True, mask_hits=False, scale=2.0, chunk=128, **SHAPE), 9)[:7] == (2, 4, 5, 2.0, 0.0, 128, DEV | NOL2)
    assert _tail(run(rt, "inbatch_step", l2_reg=0.125, **SHAPE), 5)[:3] == (0.125, 0, HITS)
    o = run(rt, "inbatch_loss", bias=False, mask_hits=False, per_row=True)
    assert o.only_call()[1][3] is None and o.only_call()[1][10] == 0 and o.only_call()[1][-1] == o.result[2].ctypes.data and o.result[2].shape == (9,)
    assert _tail(run(rt, "LightGCN.step", True, l2_reg=0.5, train="item", want_loss=False), 5) == (0.5, 2, DEV, None, None)
    assert run(rt, "LightGCN.step", True, want_loss=False).calls[-1][0] == "orx_lightgcn_step"          # (no index check without the loss)
    assert _tail(run(rt, "VBPR.step", l2_reg=0.5, l2_proj=0.25, batch_chunk=64, train=("proj", "user"), **SHAPE), 7)[:5] == (0.5, 0.25, 64, 9, 0)
    assert run(rt, "VBPR.step", bias=False, **SHAPE).only_call()[1][4] is None
    assert _tail(run(rt, "SeqRec.step", l2_reg=0.5, train=("history", "bias"), loss="logsig"), 5)[:3] == (0.5, 5, 0)
    assert run(rt, "SeqRec.step", bias=False).only_call()[1][5] is None and run(rt, "SeqRec.loss", bias=False).only_call()[1][4] is None


# ---- 2. the defaults ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,at", [("pairwise_step", 9), ("pointwise_step", 10), ("multineg_step", 11), ("inbatch_step", 9), ("VBPR.step", 13)])
def test_defaults_of_the_k_step_calls(entry, at):
    """`at`: where K stands in the C call; B = None is len // K, id_stride = None is B, K = 0 is the library's no-op"""
    shape = lambda o: tuple(o.only_call()[1][i] for i in ((at, at + 1, at + 3) if entry == "multineg_step" else (at, at + 1, at + 2)))
    assert shape(run(rt, entry)) == (1, 9, 9)
    assert shape(run(rt, entry, K=2)) == (2, 4, 4)
    assert shape(run(rt, entry, K=2, B=3)) == (2, 3, 3)
    assert shape(run(rt, entry, K=2, B=3, id_stride=6)) == (2, 3, 6)
    assert shape(run(rt, entry, True, n=10, K=3, id_stride=4, B=2)) == (3, 2, 4)
    assert shape(run(rt, entry, K=1, B=0)) == (1, 0, 0)
    if entry in OVERLAP:          # a stride below B reaches the library as it is: overlapping windows, one batch K times
        assert shape(run(rt, entry, n=8, K=3, B=4, id_stride=2)) == (3, 4, 2)
        assert shape(run(rt, entry, True, n=4, K=3, B=4, id_stride=0)) == (3, 4, 0)
        assert shape(run(rt, entry, n=4, K=1, B=4, id_stride=0)) == (1, 4, 0) and shape(run(rt, entry, n=4, K=1, B=4, id_stride=-7)) == (1, 4, -7)
    for kw in (dict(K=0), dict(K=0, B=4), dict(K=0, n=0)):
        o = run(rt, entry, **kw)
        assert shape(o)[0] == 0 and shape(o)[1:] == ((4, 4) if "B" in kw else (0, 0))
        assert len(o.result) == 2 and all(x.shape == (0,) and x.dtype == np.float32 for x in o.result)
        assert run(rt, entry, want_loss=False, **kw).result is None


# ---- 3. the refusals ---------------------------------------------------------------------------------------------------------------------
def refused(entry, *a, **kw):
    o = run(rt, entry, *a, **kw)
    assert isinstance(o.error, ValueError), (entry, kw, repr(o.error))
    assert entry in str(o.error), str(o.error)
    assert o.calls == [], o.calls
    return str(o.error)


def second_list(entry):
    return "iid" if entry.startswith("pointwise") else "pid"


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_mixed_sides_and_unequal_lengths_are_refused(entry, dev):
    name = second_list(entry)
    assert "ids must be all on the host or all on the device" in refused(entry, dev, over={name: dict(dev=not dev)}, **shape_kw(entry))
    last = "label" if entry.startswith("pointwise") else "nid" if "nid" in si.make_lists(entry, False, 1) else name
    for which in {name, last}:
        shape = (NEED + 1, N) if which == "nid" and si.family(entry) in ("multineg", "SeqRec") else (NEED + 1,)
        refused(entry, dev, over={which: dict(shape=shape)}, **shape_kw(entry))
    if last == "label":
        assert "label on the" in refused(entry, dev, over={"label": dict(dev=not dev)}, **shape_kw(entry))


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("entry", KSTEP)
def test_lists_one_short_of_what_the_steps_read_are_refused(entry, dev):
    refused(entry, dev, n=NEED - 1, optional=si.OPTIONAL, **SHAPE)
    assert run(rt, entry, dev, n=NEED, optional=si.OPTIONAL, **SHAPE).error is None
    refused(entry, dev, K=-1)
    refused(entry, dev, B=-1)
    if entry in OVERLAP:          # steps may share ids; only a stride that steps in front of the lists is refused
        refused(entry, dev, K=2, B=4, id_stride=-1)
        refused(entry, dev, n=NEED - 3, K=3, B=4, id_stride=2)          # (needs 8)
    else:
        refused(entry, dev, K=2, B=4, id_stride=3)
        refused(entry, dev, K=1, B=4, id_stride=0)


@pytest.mark.parametrize("entry,name", [(e, nm) for e in ENTRIES for nm in si.OPTIONAL if nm in [x[0] for x in si._LISTS[si.family(e)]]])
def test_float_lists_on_the_wrong_side_or_of_the_wrong_length_are_refused(entry, name):
    kw = shape_kw(entry)
    like_nid = name == "neg_offset"
    full = NEED * N if like_nid else ITEMS if name == "item_offset" and entry in FULL else NEED          # (the full softmax: one float per ITEM)
    assert f"{name} on the device with ids on the host" in refused(entry, False, over={name: dict(dev=True)}, **kw)
    assert f"{name} on the host with ids on the device" in refused(entry, True, over={name: dict(dev=False)}, **kw)
    for dev in (False, True):
        msg = refused(entry, dev, over={name: dict(shape=(NEED, N - 1) if like_nid else (full - 1,))}, **kw)
        assert f"{NEED * (N - 1) if like_nid else full - 1} {name} for {full} ids" in msg


@pytest.mark.parametrize("entry", ["pairwise_step", "pointwise_step", "LightGCN.step", "VBPR.step", "SeqRec.step"])
def test_a_bad_train_is_refused(entry):
    kw = shape_kw(entry)
    assert "unknown" in refused(entry, train=("users",), **kw) and "unknown" in refused(entry, train="all", **kw)
    assert "empty" in refused(entry, train=(), **kw)
    assert '"bias" named' in refused(entry, train=("item", "bias"), bias=False, **kw)
    other = {"VBPR.step": "history", "SeqRec.step": "user"}.get(entry, "proj")          # a name of another family's dictionary
    assert "unknown" in refused(entry, train=("item", other), **kw)


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf"), -float("inf")])
@pytest.mark.parametrize("entry,name", [(e, "l2_reg") for e in STEPS + ("LightGCN.loss",)] + [("VBPR.step", "l2_proj"), ("DeepSeqRec.step_full", "l2_mlp")])
def test_a_bad_coefficient_is_refused(entry, name, bad):
    assert f"{name} must be finite and >= 0" in refused(entry, **{name: bad}, **shape_kw(entry))


def test_no_l2_with_an_l2_reg_of_the_callers_own_is_refused():
    for entry, l2 in (("pairwise_step", 0.01), ("pairwise_step", 1.0), ("pointwise_step", 0.01), ("multineg_step", 0.5), ("inbatch_step", 0.5)):
        assert "no_l2" in refused(entry, no_l2=True, l2_reg=l2, **SHAPE)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("entry", ["multineg_step", "multineg_loss", "SeqRec.step", "SeqRec.loss"])
def test_a_bad_loss_kind_or_shape_of_the_negatives_is_refused(entry, dev):
    kw = shape_kw(entry)
    assert "unknown loss" in refused(entry, dev, loss="hinge", **kw)
    assert "nid must be an array shaped" in refused(entry, dev, over={"nid": dict(shape=(NEED * N,))}, **kw)
    assert "N = 0" in refused(entry, dev, over={"nid": dict(shape=(NEED, 0))}, **kw)
    assert "N = 65" in refused(entry, dev, over={"nid": dict(shape=(NEED, 65))}, **kw)
    assert run(rt, entry, dev, over={"nid": dict(shape=(NEED, 64))}, **kw).error is None
    o = run(rt, entry, dev, over={"nid": dict(shape=(1, NEED, N))}, **kw)          # [..., B, N] for the one, exactly [B, N] for the other
    assert (o.error is None) if entry.startswith("multineg") else isinstance(o.error, ValueError)
    assert "nid must be" in refused(entry, dev, over={"nid": rt.DevicePtr(0x1000, NEED * N)}, **kw)


def test_the_tables_of_a_dot_product_family_are_checked_once():
    T = lambda rows, dim: si.StandinTable(None, "x", rows, dim)
    for what, user_dim, item_dim, items, bias in (("dims", 8, 9, 30, None), ("rows", 8, 8, 30, T(29, 1)), ("width", 8, 8, 30, T(30, 2))):
        with pytest.raises(ValueError, match="a_call: (user dim 8 != item dim 9|bias must be \\[30, 1\\])"):
            rt._dot_tables("a_call", user_dim, item_dim, items, bias)
    rt._dot_tables("a_call", 8, 8, 30, None), rt._dot_tables("a_call", 8, 8, 30, T(30, 1))
    w = si.World(rt)
    for entry, tables in (("multineg_step", dict(U=T(20, 9))), ("multineg_loss", dict(b=T(30, 2))), ("inbatch_step", dict(U=T(20, 9))),
                          ("inbatch_loss", dict(b=T(29, 1)))):
        w = si.World(rt)
        vars(w).update(tables)
        with pytest.raises(ValueError, match=entry):
            si.call(w, entry, si.make_lists(entry, False, NEED), {})
        assert w.calls == []


# ---- 4. the library's stream waits for torch's before it reads device ids ------------------------------------------------------------------
@pytest.mark.parametrize("entry,ids", [("pairwise_loss", {"uid", "pid", "nid"}), ("pointwise_loss", {"uid", "iid", "label"})])
def test_forward_losses_order_the_stream_behind_torch_for_the_ids(entry, ids):
    o = run(rt, entry, True)
    assert o.error is None and o.ordered_lists() == ids and len(o.ordered) >= 1
    assert any(o.lists["uid"] is t for group in o.ordered for t in group)


# ---- 5. train and l2 are refused before a table, the optimizer or the context is touched ---------------------------------------------------
def test_train_and_l2_refusals_come_before_any_device_object():
    t = si.NoDevice()
    ids, lab = np.zeros(4, np.int32), np.zeros(4, np.float32)
    nid = np.zeros((4, N), np.int32)
    models = {}
    for cls, names in ((rt.LightGCN, ("U", "V", "ctx", "_h")), (rt.VBPR, ("U", "V", "b", "E", "features", "ctx")), (rt.SeqRec, ("H", "V", "b", "ctx")),
                       (rt.DeepSeqRec, ("H", "V", "b", "ctx", "side", "layers", "_tables"))):
        m = models[cls.__name__] = cls.__new__(cls)
        for nm in names:
            setattr(m, nm, t)
    steps = {
        "pairwise_step": lambda **kw: rt.pairwise_step("bpr", t, t, t, t, ids, ids, ids, **kw),
        "pointwise_step": lambda **kw: rt.pointwise_step("wrmf", t, t, t, t, None, ids, ids, lab, **kw),
        "multineg_step": lambda **kw: rt.multineg_step("softmax", t, t, t, t, ids, ids, nid, **kw),
        "inbatch_step": lambda **kw: rt.inbatch_step(t, t, t, t, ids, ids, **kw),
        "LightGCN.step": lambda **kw: models["LightGCN"].step(t, ids, ids, ids, **kw),
        "VBPR.step": lambda **kw: models["VBPR"].step(t, ids, ids, ids, **kw),
        "SeqRec.step": lambda **kw: models["SeqRec"].step(t, (np.arange(5, dtype=np.int32), ids), ids, nid, **kw),
        "fullsoftmax_step": lambda **kw: rt.fullsoftmax_step(t, t, t, t, ids, ids, **kw),
        "SeqRec.step_full": lambda **kw: models["SeqRec"].step_full(t, (np.arange(5, dtype=np.int32), ids), ids, **kw),
        "DeepSeqRec.step_full": lambda **kw: models["DeepSeqRec"].step_full(t, (np.arange(5, dtype=np.int32), ids), ids, **kw),
    }
    assert set(steps) == set(STEPS)
    for entry, step in steps.items():
        for kw in (dict(l2_reg=-1.0), dict(l2_reg=math.nan)) + ((dict(train=("users",)), dict(train=())) if entry[0] not in "mi" else ()):
            with pytest.raises(ValueError, match=entry):
                step(**kw)
    for entry in ("pairwise_step", "pointwise_step", "multineg_step", "inbatch_step"):
        with pytest.raises(ValueError, match="no_l2"):
            steps[entry](no_l2=True, l2_reg=0.01)
    for bad in (-1.0, math.nan):
        with pytest.raises(ValueError, match="DeepSeqRec.step_full: l2_mlp"):
            steps["DeepSeqRec.step_full"](l2_mlp=bad)


# ---- 6. the calls on the softmax over all items: label sets, the tower's arrays, the options --------------------------------------------------
BAGS = ("SeqRec.step_full", "SeqRec.loss_full", "DeepSeqRec.step_full", "DeepSeqRec.loss_full")


@pytest.mark.parametrize("dev,f", [(False, 0), (True, DEV)], ids=["host", "device"])
@pytest.mark.parametrize("lw", [True, False], ids=["label_weights", "no_label_weights"])
@pytest.mark.parametrize("entry", BAGS)
def test_ragged_label_sets_reach_the_sets_call_as_they_came(entry, lw, dev, f):
    o = run(rt, entry, dev, labels="ragged", optional=si.OPTIONAL + (("label_weights",) if lw else ()))
    assert_call(o, *expected_full(entry, f, labels="ragged", label_weights=lw))
    assert o.ordered_lists() == (set(o.lists) if dev else set())
    assert flushed(o) == FLUSHED[si.family(entry)]


@pytest.mark.parametrize("lw", [True, False], ids=["label_weights", "no_label_weights"])
@pytest.mark.parametrize("entry", BAGS)
def test_a_padded_pair_of_label_sets_is_made_ragged_on_the_host(entry, lw):
    """(a padded pair on the device is converted with torch's own ops: the GPU tests have it)"""
    o = run(rt, entry, False, labels="padded", optional=("label_weights",) if lw else ())
    name, want = expected_full(entry, 0, labels="ragged", label_weights=lw, optional=False)
    at = want.index("@lab_ptr")
    assert_call(o, name, tuple(OUT if str(w).startswith("@lab") else w for w in want))          # (arrays of the wrapper's own, 18 entries)
    got = o.only_call()[1]
    assert not {got[at], got[at + 1], got[at + 2]} & {o.pointer_of(k) for k in o.lists} and got[at] != got[at + 1]
    assert flushed(o) == FLUSHED[si.family(entry)]


@pytest.mark.parametrize("dev,f", [(False, 0), (True, DEV)], ids=["host", "device"])
@pytest.mark.parametrize("entry", FULL)
def test_the_options_of_the_full_softmax_calls(entry, dev, f):
    step, deep = "step" in entry, entry.startswith("Deep")
    o = run(rt, entry, dev, bias=False, scale=2.0, chunk_items=128)
    assert_call(o, *expected_full(entry, f, optional=False, bias=False, scale=2.0, chunks=(128, 0)))
    if not step:
        if not dev:          # (device lists: the rows are a torch tensor on the device -- the GPU tests have it)
            o = run(rt, entry, dev, per_row=True)
            name, args = o.only_call()
            assert len(o.result) == 3 and all(isinstance(x, float) for x in o.result[:2])
            assert args[-1] == o.result[2].ctypes.data and o.result[2].shape == (NEED,) and o.result[2].dtype == np.float32
        return
    role = "user" if entry.startswith("fullsoftmax") else "history"
    o = run(rt, entry, dev, l2_reg=0.5, chunk_samples=64, train=(role, "bias"), want_loss=False, **(dict(l2_mlp=0.25) if deep else {}))
    assert_call(o, *expected_full(entry, f, optional=False, l2=(0.5, 0.25), chunks=(0, 64), mask=5, outs=(None, None)))
    assert o.result is None and [t.name for t in o.world.opt._tables] == [c for c in (["U", "V", "b"] if role == "user" else
                                                                                       ["H", "V", "b"] + (["S0", "S1", "W0", "c0", "W1"] if deep else []))]
    if deep:
        assert _tail(run(rt, entry, dev, train=("side", "tower")), 4)[0] == _ffi.ORX_TRAIN_SIDE | _ffi.ORX_TRAIN_TOWER


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("entry", BAGS)
def test_what_the_label_and_side_lists_refuse(entry, dev):
    deep = entry.startswith("Deep")
    assert "either pid" in refused(entry, dev, labels="ragged", over={"pid": {}}) and "not both" in refused(entry, dev, labels="ragged", over={"pid": {}})
    o = run(rt, entry, dev, over={"pid": None})
    assert isinstance(o.error, ValueError) and "one of them" in str(o.error) and o.calls == []
    assert "label_weights without labels" in refused(entry, dev, optional=("label_weights",), over={"label_weights": dict(shape=(NEED,))})
    assert "must live where the bags live" in refused(entry, dev, labels="ragged", over={"lab_ptr": dict(dev=not dev), "lab_items": dict(dev=not dev)})
    assert f"{NEED} bags and {NEED + 1} label sets" in refused(entry, dev, labels="ragged", over={"lab_ptr": dict(shape=(NEED + 2,)), "lab_items": dict(shape=(2 * NEED + 2,))})
    assert f"{2 * NEED - 1} label_weights for {2 * NEED} ids" in refused(entry, dev, labels="ragged", optional=("label_weights",),
                                                                         over={"label_weights": dict(shape=(2 * NEED - 1,))})
    assert "label_weights on the" in refused(entry, dev, labels="ragged", optional=("label_weights",), over={"label_weights": dict(dev=not dev)})
    assert f"{NEED} bags and {NEED - 1} label ids" in refused(entry, dev, over={"pid": dict(shape=(NEED - 1,))})
    if not dev:
        assert "label_weights [9, 2] beside padded labels [9, 3]" in refused(entry, dev, labels="padded", optional=("label_weights",),
                                                                             over={"label_weights": dict(shape=(NEED, 2))})
        bad = np.arange(NEED + 1, dtype=np.int32) * 2
        bad[-1] -= 1
        assert "bag offsets must start at 0" in refused(entry, dev, over={"ptr": bad})
    if deep:
        assert "1 side id lists for 2 side tables" in refused(entry, dev, side_ids=(np.zeros(NEED, np.int32),))
        assert "ids must be all on the host or all on the device" in refused(entry, dev, over={"f1": dict(dev=not dev)})
        assert "side id lists of" in refused(entry, dev, over={"f0": dict(shape=(NEED + 1,))})
        if "step" in entry:
            o = run(rt, entry, dev, train=("side",))
            assert o.error is None


def test_a_bad_train_of_the_full_softmax_steps_is_refused():
    for entry in ("fullsoftmax_step", "SeqRec.step_full", "DeepSeqRec.step_full"):
        assert "unknown" in refused(entry, train=("users",)) and "empty" in refused(entry, train=())
        assert '"bias" named' in refused(entry, train=("item", "bias"), bias=False)
        assert "unknown" in refused(entry, train=("item", "history" if entry == "fullsoftmax_step" else "user"))
    assert "unknown" in refused("SeqRec.step_full", train=("tower",))
    m = rt.DeepSeqRec.__new__(rt.DeepSeqRec)
    m.H = m.V = m.ctx = si.NoDevice()
    m.b, m.side = None, []
    with pytest.raises(ValueError, match='DeepSeqRec.step_full: train: "side" named'):
        m.step_full(si.NoDevice(), (np.arange(5, dtype=np.int32), np.zeros(4, np.int32)), np.zeros(4, np.int32), train=("side",))
