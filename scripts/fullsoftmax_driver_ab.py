"""Bits and host-time A/B of the ten full-softmax entry points between two trees (the parent's per-form host skeletons against
the shared drivers of api_fullsoftmax.hip), one tree per process:

    python scripts/fullsoftmax_driver_ab.py bits TREE OUT       three steps and the forward of every case on TREE's library; one line
                                                                per array to OUT: case, array, shape, sha256 of its bytes -- every
                                                                table, every optimizer slot, (loss, l2) of each step and of the
                                                                forward, the per-row losses; then the launches per kernel
                                                                (Context.prof_get) of one call of each entry point
    python scripts/fullsoftmax_driver_ab.py time TREE OUT       wall microseconds per call of each entry point, device lists,
                                                                want_loss=False, at the small shape (B = 256, items = 4096, D = 64:
                                                                launches dominate) and at the benchmarks' (B = 4096, D = 64, 100000
                                                                items, bags and label sets of 20); one JSON line to OUT
    python scripts/fullsoftmax_driver_ab.py table P.. -- C..    the time files of the parent's processes and of the change's -- or the
                                                                JSON lines of a benchmark script's measuring processes: every
                                                                median in them -- as the tables of profiles/fullsoftmax_driver_ab.txt
    python scripts/fullsoftmax_driver_ab.py compare A B [C]     A and B (two runs of one tree) must agree everywhere; C (the other tree)
                                                                must equal A in every line -- prints the counts and every difference

Run the parent twice and the change once, each process under its own timeout.  profiles/fullsoftmax_driver_ab.txt is such a
comparison.  These kernels use no float atomics, so two runs of one tree agree in every bit."""
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

OPTS = ("sgd", "adagrad", "adam", "momentum")
TOWERS = {"t0": dict(side=(), hidden=()), "t2": dict(side=((7, 3), (5, 2)), hidden=(12, 9))}          # 0 side / 1 layer; 2 side / 3 layers, layer 1 without a bias


def load(tree):
    sys.path.insert(0, os.path.abspath(tree))
    from openrec_amd import runtime as rt
    assert os.path.abspath(rt.__file__).startswith(os.path.abspath(tree) + os.sep), rt.__file__
    return rt


def make_opt(rt, name, ctx):
    return {"sgd": lambda: rt.Optimizer.sgd(0.05, ctx=ctx), "adagrad": lambda: rt.Optimizer.adagrad(0.05, ctx=ctx),
            "adam": lambda: rt.Optimizer.adam(0.01, ctx=ctx), "momentum": lambda: rt.Optimizer.momentum(0.05, 0.9, ctx=ctx)}[name]()


def cases():
    """-> [dict]: family, opt, dev, want_loss, train, B, items, D, chunks, bags (normal | one_empty | all_empty), lw, empty_set, tower"""
    out = []

    def add(family, opt="sgd", dev=False, want_loss=True, train=None, B=63, items=65, D=8, chunks=(0, 0), bags="normal", lw=False, empty_set=False,
            tower="t2", minus_inf=True):
        out.append(dict(family=family, opt=opt, dev=dev, want_loss=want_loss, train=train, B=B, items=items, D=D, chunks=chunks, bags=bags, lw=lw,
                        empty_set=empty_set, tower=tower, minus_inf=minus_inf))

    for fam in ("user", "seq", "seq_sets", "tower", "tower_sets"):
        role = "user" if fam == "user" else "history"
        k = 0
        for opt in OPTS:          # optimizer x lists x losses
            for dev in (False, True):
                for want in (True, False):
                    add(fam, opt, dev, want, lw=bool(k & 1), tower=("t0", "t2")[k >> 1 & 1], bags=("normal", "one_empty")[k >> 2 & 1])
                    k += 1
        masks = [(role,), ("item",), ("bias",), (role, "bias")] + ([("side",), ("tower",), ("side", "tower")] if fam.startswith("tower") else [])
        for opt in ("sgd", "adam"):          # each single-table mask and a two-table one
            for i, m in enumerate(masks):
                add(fam, opt, bool(i & 1), True, train=m, lw=True)
        for i, (B, items, D) in enumerate([(1, 65, 8), (1, 300, 50), (63, 300, 8), (200, 65, 50), (200, 300, 8), (200, 300, 50)]):          # shapes
            add(fam, OPTS[i % 4], bool(i & 1), True, B=B, items=items, D=D, chunks=(64, 64) if B == 200 else (0, 0), lw=bool(i & 2), tower=("t2", "t0")[i & 1])
        if fam != "user":
            for opt in ("sgd", "adam"):          # n = 0 with the history table trained, then with it frozen
                add(fam, opt, opt == "adam", True, bags="all_empty")
                add(fam, opt, opt == "sgd", False, bags="all_empty", train=("history",))
                add(fam, opt, False, True, bags="all_empty", train=("item",))
        if fam.endswith("sets"):
            for dev in (False, True):
                add(fam, "adam", dev, True, empty_set=True, lw=dev)
        add(fam, "adagrad", True, True, minus_inf=False)
    return out


def name_of(c):
    return "{family}/{opt}/{lists}/{loss}/train={train}/B{B}i{items}D{D}c{chunks}/{bags}/lw{lw}/es{empty_set}/{tower}/inf{minus_inf}".format(
        **{**c, "lists": "dev" if c["dev"] else "host", "loss": "loss" if c["want_loss"] else "noloss", "train": "+".join(c["train"]) if c["train"] else "all",
           "chunks": "%d_%d" % c["chunks"], "lw": int(c["lw"]), "empty_set": int(c["empty_set"]), "minus_inf": int(c["minus_inf"])})


class Model:
    """one case's tables, optimizer and batches, from a seed that depends on the case alone"""

    def __init__(self, rt, ctx, c, seed):
        self.rt, self.ctx, self.c = rt, ctx, c
        rng = self.rng = np.random.default_rng(seed)
        items, D, fam = c["items"], c["D"], c["family"]
        T = lambda rows, dim: rt.Table(rows, dim, ctx).write(rng.uniform(-0.3, 0.3, (rows, dim)).astype(np.float32))
        self.tables = {"V": T(items, D), "b": T(items, 1)}
        self.opt = make_opt(rt, c["opt"], ctx)
        if fam == "user":
            self.tables["U"] = T(40, D)
        else:
            Dh = D if not fam.startswith("tower") else 6
            self.tables["H"] = T(items, Dh)
        if fam.startswith("tower"):
            tw = TOWERS[c["tower"]]
            side = [T(r, d) for r, d in tw["side"]]
            widths = [sum(d for _, d in tw["side"]) + 6, *tw["hidden"], D]
            layers = []
            for l in range(len(widths) - 1):
                W = T(widths[l], widths[l + 1])
                cb = None if l == 1 else T(1, widths[l + 1])
                layers.append((W, cb))
                self.tables[f"W{l}"] = W
                if cb is not None:
                    self.tables[f"c{l}"] = cb
            for j, s in enumerate(side):
                self.tables[f"S{j}"] = s
            self.side = side
            self.model = rt.DeepSeqRec(self.tables["H"], self.tables["V"], self.tables["b"], layers, side=side, pool="mean", relu_last=False)
        elif fam != "user":
            self.model = rt.SeqRec(self.tables["H"], self.tables["V"], self.tables["b"], pool=("fixed", 3.0))

    def to(self, x):
        if not self.c["dev"] or x is None:
            return x
        import torch
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()

    def batch(self):
        """the keyword arguments of one call, fresh lists from the case's stream"""
        c, rng = self.c, self.rng
        B, items, fam = c["B"], c["items"], c["family"]
        kw = {}
        off = rng.normal(0, 0.5, items).astype(np.float32)
        if c["minus_inf"]:
            off[items - 3:] = -np.inf          # (no label among them: a removed label is an infinite loss, and NaN tables tell nothing apart)
        kw["item_offset"] = self.to(off)
        kw["weights"] = self.to(rng.uniform(0.5, 1.5, B).astype(np.float32))
        pid = rng.integers(0, items - 3, B).astype(np.int32)
        if fam == "user":
            self.ids = (self.to(rng.integers(0, 40, B).astype(np.int32)), self.to(pid))
            return kw
        ln = rng.integers(1, 6, B) if not c.get("bag") else np.full(B, c["bag"])
        if c["bags"] == "one_empty":
            ln[B // 2] = 0
        if c["bags"] == "all_empty":
            ln[:] = 0
        ptr = np.zeros(B + 1, np.int32)
        ptr[1:] = np.cumsum(ln)
        self.bags = (self.to(ptr), self.to(rng.integers(0, items, int(ptr[-1])).astype(np.int32)))
        if fam.endswith("sets"):
            ll = rng.integers(1, 5, B) if not c.get("bag") else np.full(B, c["bag"])
            if c["empty_set"]:
                ll[0] = 0
            lp = np.zeros(B + 1, np.int32)
            lp[1:] = np.cumsum(ll)
            kw["labels"] = (self.to(lp), self.to(rng.integers(0, items - 3, int(lp[-1])).astype(np.int32)))
            if c["lw"]:
                kw["label_weights"] = self.to(rng.uniform(0.5, 2.0, int(lp[-1])).astype(np.float32))
        else:
            kw["pid"] = self.to(pid)
        if fam.startswith("tower"):
            kw["side_ids"] = tuple(self.to(rng.integers(0, s.rows, B).astype(np.int32)) for s in self.side)
        return kw

    def step(self, kw, want_loss):
        c = self.c
        more = dict(scale=1.5, l2_reg=0.01, train=c["train"], chunk_items=c["chunks"][0], chunk_samples=c["chunks"][1], want_loss=want_loss)
        if c["family"] == "user":
            return self.rt.fullsoftmax_step(self.opt, self.tables["U"], self.tables["V"], self.tables["b"], *self.ids, **kw, **more)
        if c["family"].startswith("tower"):
            more["l2_mlp"] = 0.02
        return self.model.step_full(self.opt, self.bags, **kw, **more)

    def forward(self, kw, per_row=True):
        more = dict(scale=1.5, chunk_items=self.c["chunks"][0], per_row=per_row)
        if self.c["family"] == "user":
            return self.rt.fullsoftmax_loss(self.tables["U"], self.tables["V"], self.tables["b"], *self.ids, **kw, **more)
        return self.model.loss_full(self.bags, **kw, **more)


def digest(x):
    a = np.ascontiguousarray(x)
    return f"{list(a.shape)} {hashlib.sha256(a.tobytes()).hexdigest()[:24]}"


def bits(tree, out_path):
    rt = load(tree)
    ctx = rt.Context(0)
    lines = []
    every = cases()
    for i, c in enumerate(every):
        m, nm = Model(rt, ctx, c, 1000 + i), name_of(c)
        for s in range(3):
            kw = m.batch()
            r = m.step(kw, c["want_loss"])
            if r is not None:
                lines.append(f"{nm} step{s}.losses {digest(np.concatenate(r))}")
        fwd = m.forward(kw)
        lines.append(f"{nm} forward.losses {digest(np.array(fwd[:2], np.float32))}")
        lines.append(f"{nm} forward.rows {digest(fwd[2])}")
        for tn, t in sorted(m.tables.items()):
            lines.append(f"{nm} table.{tn} {digest(t.read())}")
            for k in range(rt.Optimizer.NSLOTS[c["opt"]]):
                try:
                    lines.append(f"{nm} slot{k}.{tn} {digest(m.opt.slot(t, k))}")
                except Exception as e:          # (a table the optimizer holds no slots for)
                    lines.append(f"{nm} slot{k}.{tn} none:{type(e).__name__}")
    # the launches of one call of each entry point
    for fam in ("user", "seq", "seq_sets", "tower", "tower_sets"):
        c = next(x for x in every if x["family"] == fam and x["opt"] == "adam" and x["dev"] and x["train"] is None and x["bags"] == "normal")
        m = Model(rt, ctx, c, 7)
        kw = m.batch()
        m.step(kw, True)
        for what, call in (("step", lambda: m.step(kw, True)), ("loss", lambda: m.forward(kw, False))):
            ctx.synchronize(); ctx.prof_enable(True); ctx.prof_reset()
            call()
            ctx.synchronize()
            got = {k: v["launches"] for k, v in ctx.prof_get().items() if v["launches"]}
            ctx.prof_enable(False)
            lines.append(f"launches {fam}.{what} {json.dumps(got, sort_keys=True)}")
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(every)} cases, {len(lines)} lines -> {out_path}")


def timed(tree, out_path, reps=5):
    rt = load(tree)
    import torch
    ctx = rt.Context(0)
    res = {}
    for shape, calls, kw0 in (("small", 300, dict(B=256, items=4096, D=64)), ("bench", 20, dict(B=4096, items=100_000, D=64, bag=20))):
        for fam in ("user", "seq", "seq_sets", "tower", "tower_sets"):
            c = dict(family=fam, opt="adam", dev=True, want_loss=False, train=None, chunks=(0, 0), bags="normal", lw=False, empty_set=False, tower="t2",
                     minus_inf=False, **kw0)
            m = Model(rt, ctx, c, 5)
            kw = m.batch()
            for what, call in (("step", lambda: m.step(kw, False)), ("loss", lambda: m.forward(kw, False))):
                us = []
                for r in range(reps + 1):          # (the first repetition warms up and is dropped)
                    ctx.synchronize(); torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        call()
                    ctx.synchronize()
                    us.append((time.perf_counter() - t0) / calls * 1e6)
                res[f"{shape}.{fam}.{what}"] = round(statistics.median(us[1:]), 2)
    with open(out_path, "w") as f:
        f.write(json.dumps(res, sort_keys=True) + "\n")
    print(json.dumps(res, sort_keys=True))


def table(parent_files, change_files):
    def flat(d, at=""):          # a benchmark script's nested result: its medians, named by their path
        if not isinstance(d, dict):
            return {}
        if not any(isinstance(v, dict) for v in d.values()) and "." not in at and all(isinstance(v, (int, float)) for v in d.values()):
            return d
        out = {}
        for k, v in d.items():
            if isinstance(v, dict):
                out.update(flat(v, f"{at}{k}."))
            elif "median" in k and isinstance(v, (int, float)):
                out[at + k] = v
        return out
    P, C = [flat(json.load(open(p))) for p in parent_files], [flat(json.load(open(p))) for p in change_files]
    print(f"wall microseconds per call, median of 5 repetitions per process; {len(P)} parent and {len(C)} change processes, alternating")
    for k in sorted(P[0]):
        p, c = sorted(x[k] for x in P), sorted(x[k] for x in C)
        mp, mc = statistics.median(p), statistics.median(c)
        w = max(26, max(len(x) for x in P[0]))
        f = (lambda v: f"{v:9.4f}") if p[-1] < 100 else (lambda v: f"{v:9.2f}")          # (milliseconds below 100 keep four decimals)
        print(f"{k:{w}s} parent {f(p[0])} .. {f(p[-1])} ({100 * (p[-1] - p[0]) / p[0]:4.1f} %)  change {f(c[0])} .. {f(c[-1])}  median p {f(mp)} c {f(mc)}"
              f"  {'inside' if p[0] <= mc <= p[-1] else 'BELOW' if mc < p[0] else 'ABOVE'} the parent's range")


def compare(a, b, c=None):
    rd = lambda p: {" ".join(ln.split(" ", 2)[:2]): ln.rstrip("\n") for ln in open(p)}          # case and array -> the line
    A, B = rd(a), rd(b)
    unstable = sorted(k for k in A if A[k] != B.get(k))
    print(f"{len(A)} lines in {a}; {len(unstable)} differ between the two runs of one tree")
    for k in unstable:
        print("  unstable:", k)
    if c:
        C = rd(c)
        diff = sorted(k for k in set(A) | set(C) if k not in unstable and A.get(k) != C.get(k))
        print(f"{len(C)} lines in {c}; {len(diff)} differ from {a} outside the unstable ones")
        for k in diff:
            print("  differs:", A.get(k), "|", C.get(k))
        return 1 if diff else 0
    return 0


if __name__ == "__main__":
    if len(sys.argv) < 4 or sys.argv[1] not in ("bits", "time", "compare", "table"):
        sys.exit(__doc__)
    if sys.argv[1] == "table":
        at = sys.argv.index("--")
        sys.exit(table(sys.argv[2:at], sys.argv[at + 1:]))
    if sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:5]))
    (bits if sys.argv[1] == "bits" else timed)(sys.argv[2], sys.argv[3])
