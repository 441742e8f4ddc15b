"""A/B of the runtime's train-step wrappers between two trees, on the recording stand-in of tests/runtime_standin.py (no
library, no device):

    python scripts/runtime_args_ab.py dump TREE     one line per call of a fixed table: the C call that TREE's
                                                    openrec_amd.runtime made, every pointer named after the list it came from,
                                                    or the type of the exception it raised
    python scripts/runtime_args_ab.py time TREE     the host time of TREE's wrapper alone, microseconds per call

Run both on a checkout of the parent commit (git worktree add DIR HEAD~1) and on this tree and compare: `diff` of the two dumps,
and the two time tables side by side.  profiles/runtime_args_ab.txt is such a comparison.  The stand-in always comes from the tree
this script lies in; only openrec_amd is TREE's."""
import os
import platform
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(tree):
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, os.path.abspath(tree))
    import runtime_standin as si
    from openrec_amd import runtime as rt
    assert os.path.abspath(rt.__file__).startswith(os.path.abspath(tree) + os.sep), rt.__file__
    return si, rt


def cases(si):
    """-> [(label, entry, dev, kwargs of si.run)]: the cases of tests/test_runtime_args_cpu.py, then generated ones"""
    import numpy as np
    K, B, S, N, NEED = si.K, si.B, si.STRIDE, si.N, si.NEED
    kstep = ("pairwise_step", "pointwise_step", "multineg_step", "inbatch_step", "VBPR.step")
    shape = lambda e: dict(K=K, B=B, id_stride=S) if e in kstep else {}
    second = lambda e: "iid" if e.startswith("pointwise") else "pid"
    out = []
    add = lambda label, entry, dev, **kw: out.append((label, entry, dev, kw))
    for dev in (False, True):
        for e in si.ENTRIES:
            add("every optional list", e, dev, optional=si.OPTIONAL, **shape(e))
            add("no optional list", e, dev, **shape(e))
            add("no bias", e, dev, bias=False, **shape(e))
            add("mixed sides", e, dev, over={second(e): dict(dev=not dev)}, **shape(e))
            add("second list one longer", e, dev, over={second(e): dict(shape=(NEED + 1,))}, **shape(e))
            third = "label" if e.startswith("pointwise") else "nid" if "nid" in [x[0] for x in si._LISTS[si.family(e)]] else None
            if third:
                n_wide = si.family(e) in ("multineg", "SeqRec")
                add("third list one longer", e, dev, over={third: dict(shape=(NEED + 1, N) if n_wide else (NEED + 1,))}, **shape(e))
            if third == "label":
                add("label on the other side", e, dev, over={"label": dict(dev=not dev)}, **shape(e))
            for name in si.OPTIONAL:
                if name in [x[0] for x in si._LISTS[si.family(e)]]:
                    add(f"{name} on the other side", e, dev, over={name: dict(dev=not dev)}, **shape(e))
                    add(f"{name} one short", e, dev, over={name: dict(shape=(NEED, N - 1) if name == "neg_offset" else (NEED - 1,))}, **shape(e))
            if si.family(e) in ("multineg", "SeqRec"):
                add("loss kind unknown", e, dev, loss="hinge", **shape(e))
                add("loss logsig", e, dev, loss="logsig", **shape(e))
                for label, shp in (("nid flat", (NEED * N,)), ("N = 0", (NEED, 0)), ("N = 65", (NEED, 65)), ("N = 64", (NEED, 64)), ("nid [1, B, N]", (1, NEED, N))):
                    add(label, e, dev, over={"nid": dict(shape=shp)}, **shape(e))
        for e in kstep:
            add("lists one short of (K - 1) * id_stride + B: the steps read past the end", e, dev, n=NEED - 1, optional=si.OPTIONAL, **shape(e))
            for label, kw in (("defaults", {}), ("K = 2", dict(K=2)), ("K = 2, B = 3", dict(K=2, B=3)), ("K = 2, B = 3, id_stride = 6", dict(K=2, B=3, id_stride=6)),
                              ("K = 0, B = None", dict(K=0)), ("K = 0, B = None, no loss", dict(K=0, want_loss=False)), ("K = 0, B = 4", dict(K=0, B=4)),
                              ("K = 1, B = 0", dict(K=1, B=0)), ("no loss", dict(K=2, want_loss=False)),
                              ("overlapping steps: K = 3, B = 4, id_stride = 2, 8 ids", dict(n=8, K=3, B=4, id_stride=2)),
                              ("one batch K times: K = 3, B = 4, id_stride = 0, 4 ids", dict(n=4, K=3, B=4, id_stride=0)),
                              ("K = 1, B = 4, id_stride = 0, 4 ids", dict(n=4, K=1, B=4, id_stride=0)),
                              ("K = 3, B = 4, id_stride = 2, 7 ids: the steps read past the end", dict(n=7, K=3, B=4, id_stride=2)),
                              ("K = 2, B = 4, id_stride = -1: the steps read in front of the lists", dict(K=2, B=4, id_stride=-1))):
                add(label, e, dev, **kw)
        for e in si.STEPS:
            for bad in (-1.0, float("nan"), float("inf")):
                add(f"l2_reg = {bad}", e, dev, l2_reg=bad, **shape(e))
            add("l2_reg = 0.25", e, dev, l2_reg=0.25, **shape(e))
            if e.split("_")[0] not in ("multineg", "inbatch"):
                role = "history" if "SeqRec" in e else "user"
                for label, kw in (("train unknown", dict(train=("users",))), ("train empty", dict(train=())), ("train bias without a bias", dict(train=("bias",), bias=False)),
                                  (f"train {role}", dict(train=role)), ("train item and bias", dict(train=("item", "bias")))):
                    if not (e.startswith("LightGCN") and "bias" in str(kw.get("train"))):
                        add(label, e, dev, **kw, **shape(e))
            else:
                add("no_l2", e, dev, no_l2=True, **shape(e))
                add("no_l2 and l2_reg = 0.5", e, dev, no_l2=True, l2_reg=0.5, **shape(e))
        add("l2_proj = -1", "VBPR.step", dev, l2_proj=-1.0)
        add("l2_proj, batch_chunk, train proj", "VBPR.step", dev, l2_proj=0.5, batch_chunk=128, train=("proj",))
        add("l2_reg = nan", "LightGCN.loss", dev, l2_reg=float("nan"))
        for kw in (dict(), dict(no_l2=True), dict(no_l2=True, l2_reg=0.01), dict(no_l2=True, optional=("weights",)), dict(l2_reg=0.0, train=("user",)),
                   dict(model="ucml", hogwild=True, censor=True, margin=0.25), dict(model="other")):
            add("routing " + repr(kw), "pairwise_step", dev, **kw, **shape("pairwise_step"))
        for kw in (dict(no_l2=True), dict(no_l2=True, l2_reg=0.01), dict(l2_reg=0.0, train=("user",)), dict(model="gmf", sigmoid=True, hogwild=True, a=2.0, b_w=0.5),
                   dict(model="other")):
            add("routing " + repr(kw), "pointwise_step", dev, **kw, **shape("pointwise_step"))
        add("scale, chunk, no mask_hits", "inbatch_step", dev, scale=2.0, chunk=128, mask_hits=False, **shape("inbatch_step"))
        add("scale = 0", "inbatch_loss", dev, scale=0.0)
        for e in si.FULL:          # the calls on the softmax over all items
            step, bags, deep = "step" in e, "SeqRec" in e, e.startswith("Deep")
            add("scale, chunk_items", e, dev, scale=2.0, chunk_items=128)
            for label, kw in (("scale = 0", dict(scale=0.0)), ("scale = nan", dict(scale=float("nan"))), ("chunk_items = 65", dict(chunk_items=65)),
                              ("chunk_items = -64", dict(chunk_items=-64)), ("no bags", dict(n=0)), ("one bag", dict(n=1))):
                add(label, e, dev, **kw)
            if step:
                add("chunk_samples, no loss", e, dev, chunk_samples=64, want_loss=False)
                add("chunk_samples = 1", e, dev, chunk_samples=1)
                add("every table by name", e, dev, train=("user" if not bags else "history", "item", "bias"))
            if deep and step:
                for label, kw in (("l2_mlp", dict(l2_mlp=0.25)), ("l2_mlp = -1", dict(l2_mlp=-1.0)), ("l2_mlp = nan, train unknown", dict(l2_mlp=float("nan"), train="x")),
                                  ("train side and tower", dict(train=("side", "tower"))), ("train tower", dict(train="tower"))):
                    add(label, e, dev, **kw)
            if deep:
                add("one side id list", e, dev, side_ids=(np.zeros(NEED, np.int32),))
                add("a side id list on the other side", e, dev, over={"f1": dict(dev=not dev)})
                add("a side id list one longer", e, dev, over={"f0": dict(shape=(NEED + 1,))})
            if not bags:
                continue
            for lw in (False, True):
                opt = ("label_weights",) if lw else ()
                add(f"ragged label sets, label_weights {lw}", e, dev, labels="ragged", optional=opt)
                add(f"ragged label sets, label_weights {lw}, every optional list, no bias", e, dev, labels="ragged", optional=si.OPTIONAL + opt, bias=False)
                if not dev:
                    add(f"padded label sets, label_weights {lw}", e, dev, labels="padded", optional=opt)
            for label, kw in (("pid and labels", dict(labels="ragged", over={"pid": {}})), ("neither pid nor labels", dict(over={"pid": None})),
                              ("label_weights without labels", dict(over={"label_weights": dict(shape=(NEED,))})),
                              ("labels on the other side", dict(labels="ragged", over={"lab_ptr": dict(dev=not dev), "lab_items": dict(dev=not dev)})),
                              ("one label set more", dict(labels="ragged", over={"lab_ptr": dict(shape=(NEED + 2,)), "lab_items": dict(shape=(2 * NEED + 2,))})),
                              ("label_weights one short", dict(labels="ragged", over={"label_weights": dict(shape=(2 * NEED - 1,))})),
                              ("label_weights on the other side", dict(labels="ragged", over={"label_weights": dict(dev=not dev)})),
                              ("pid one short", dict(over={"pid": dict(shape=(NEED - 1,))})),
                              ("padded label_weights of another shape", dict(labels="padded", over={"label_weights": dict(shape=(NEED, 2))}))):
                if not (dev and kw.get("labels") == "padded"):
                    add(label, e, dev, **kw)
    for e in si.FULL:
        if "loss" in e:
            add("per_row", e, False, per_row=True)
    add("per_row", "inbatch_loss", False, per_row=True)
    rng = np.random.default_rng(20240607)
    for _ in range(80):
        e = kstep[rng.integers(len(kstep))]
        k, b = int(rng.choice([0, 1, 2, 3])), int(rng.choice([0, 1, 4]))
        stride = [None, b, b + 1, b + 3, 0, b // 2, max(b - 1, 0)][rng.integers(7)]
        need = (k - 1) * (b if stride is None else stride) + b if k and b else 0
        n = max(0, need + int(rng.choice([0, 0, 0, 2, -1])))
        opt = tuple(nm for nm in si.OPTIONAL if rng.integers(2))
        label = f"generated K = {k}, B = {b}, id_stride = {stride}, {n} ids" + (": the steps read past the end" if n < need else "")
        add(label, e, bool(rng.integers(2)), n=n, optional=opt, K=k, B=b, id_stride=stride, want_loss=bool(rng.integers(2)))
    for _ in range(20):
        e = si.ENTRIES[rng.integers(len(si.ENTRIES))]
        if e in kstep:
            continue
        add("generated", e, bool(rng.integers(2)), n=int(rng.choice([0, 1, 5])), optional=tuple(nm for nm in si.OPTIONAL if rng.integers(2)))
    return out


def dump(tree):
    si, rt = load(tree)
    for i, (label, entry, dev, kw) in enumerate(cases(si)):
        print(f"{i:03d} {entry} [{'device' if dev else 'host'}] {label}: {si.describe(si.run(rt, entry, dev, **kw))}")


def timed(tree, calls=20000, reps=7):
    si, rt = load(tree)
    w = si.World(rt)
    dev = lambda n, dtype="int32": si.FakeDeviceTensor(n, dtype)
    rows = []
    for label, n, fn in (
            ("pairwise_step K=200 B=65536 want_loss=False", 200 * 65536,
             lambda u, p, q: rt.pairwise_step("bpr", w.opt, w.U, w.V, w.b, u, p, q, K=200, B=65536, want_loss=False)),
            ("pairwise_step K=1 B=65536 want_loss=False", 65536,
             lambda u, p, q: rt.pairwise_step("bpr", w.opt, w.U, w.V, w.b, u, p, q, K=1, B=65536, want_loss=False)),
            ("pointwise_step K=1 B=65536 want_loss=False", 65536,
             lambda u, p, q: rt.pointwise_step("wrmf", w.opt, w.U, w.V, w.b, None, u, p, q, K=1, B=65536, want_loss=False)),
            ("multineg_step K=1 B=65536 N=3 want_loss=False", 65536,
             lambda u, p, q: rt.multineg_step("softmax", w.opt, w.U, w.V, w.b, u, p, q, K=1, B=65536, want_loss=False))):
        u, p = dev(n), dev(n)
        q = dev(n, "float32") if label.startswith("pointwise") else dev((n, si.N)) if label.startswith("multineg") else dev(n)
        us = []
        for _ in range(reps + 1):          # (the first repetition warms up and is dropped)
            w.calls.clear(); w.ctx.ordered.clear()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn(u, p, q)
            us.append((time.perf_counter() - t0) / calls * 1e6)
        rows.append((label, statistics.median(us[1:]), min(us[1:]), max(us[1:])))
    cpu = next((ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")), platform.processor())
    print(f"{cpu}; Python {platform.python_version()}; {calls} calls per repetition, median (min .. max) of {reps} repetitions, microseconds per call")
    for label, med, lo, hi in rows:
        print(f"  {label:52s} {med:7.3f}  ({lo:.3f} .. {hi:.3f})")


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] not in ("dump", "time"):
        sys.exit(__doc__)
    (dump if sys.argv[1] == "dump" else timed)(sys.argv[2])
