"""The shapes the ALS tests share (tests/test_als_cpu.py proves each bound meaningful on the CPU, tests/test_gpu_als.py holds the
device to it).  Every case carries its float64 solution x64, the float32 yardstick's x32 and e32 = max|x32 - x64| / max|x64|;
the device's bound is 4 e32.  References are computed once per process and never modified."""
import functools

import numpy as np

import als_ref as ar

NU, NI = 37, 53
DIMS = (8, 50, 64, 128)
ABS = ((1.0, 1.0), (41.0, 1.0), (1.0, 0.01), (5.0, 0.0))
REGS = (0.1, 10.0)
FACTOR = 4.0                       # the device may be this many times the float32 yardstick's error away from float64
ACC_CASES = [dict(D=D, a=a, b=b, reg=reg) for D in DIMS for (a, b) in ABS for reg in REGS]


def case_id(c):
    return "D%d-a%g-b%g-reg%g" % (c["D"], c["a"], c["b"], c["reg"])


def special_csr(R, M, seed):
    """rows 0 .. 4 observe 0, 1, 2, 17 and all M columns, the others between 0 and 12 random ones -> (ptr int64, cols int32)"""
    rng = np.random.default_rng(seed)
    counts = [0, 1, 2, min(17, M), M] + [int(x) for x in rng.integers(0, min(M, 12) + 1, R - 5)]
    rows = [np.sort(rng.choice(M, n, replace=False)) for n in counts]
    ptr = np.zeros(R + 1, np.int64)
    np.cumsum(counts, out=ptr[1:])
    return ptr, np.concatenate(rows).astype(np.int32)


def tables(D, seed, nu=NU, ni=NI):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-0.5, 0.5, (nu, D)).astype(np.float32), rng.uniform(-0.5, 0.5, (ni, D)).astype(np.float32))


def _solved(F, X0, ptr, cols, conf, a, b, reg):
    x64 = ar.half_step(F, X0, ptr, cols, conf, a, b, reg)
    x32 = ar.half_step32(F, X0, ptr, cols, conf, a, b, reg)
    return dict(F=F, X0=X0, ptr=ptr, cols=cols, conf=conf, a=a, b=b, reg=reg, x64=x64, x32=x32, e32=ar.err_vs(x32, x64))


@functools.lru_cache(maxsize=None)
def accuracy_case(k):
    """case k of ACC_CASES -> {"user": half, "item": half}: the user half solves U [37, D] against V [53, D], the item half V
    against U, each over its own special_csr"""
    c = ACC_CASES[k]
    U, V = tables(c["D"], 1000 + k)
    pu, cu = special_csr(NU, NI, 2000 + k)
    pi, ci = special_csr(NI, NU, 3000 + k)
    return dict(user=_solved(V, U, pu, cu, None, c["a"], c["b"], c["reg"]),
                item=_solved(U, V, pi, ci, None, c["a"], c["b"], c["reg"]))


CONF_B = 0.5


@functools.lru_cache(maxsize=None)
def conf_case():
    """per-entry confidences at D = 50, b = 0.5: values in [b, 20], every fourth entry EQUAL to b (a zero-weight update), through
    records with duplicates -- `records` is what ALSData is given, (ptr, cols, conf) what it must merge them into"""
    rng = np.random.default_rng(77)
    U, V = tables(50, 78)
    ptr, cols = special_csr(NU, NI, 79)
    conf = rng.uniform(CONF_B, 20.0, cols.size).astype(np.float32)
    conf[::4] = CONF_B
    users = np.repeat(np.arange(NU), np.diff(ptr)).astype(np.int32)
    # every third entry arrives as two records whose confidences add up to the entry's (halves are exact in float32)
    split = np.arange(cols.size) % 3 == 0
    ru = np.concatenate([users, users[split]]); ri = np.concatenate([cols, cols[split]])
    rc = np.concatenate([np.where(split, conf / 2, conf), conf[split] / 2]).astype(np.float32)
    order = rng.permutation(ru.size)
    records = np.zeros(ru.size, dtype=[("user_id", np.int32), ("item_id", np.int32)])
    records["user_id"], records["item_id"] = ru[order], ri[order]
    out = _solved(V, U, ptr, cols, conf, 1.0, CONF_B, 0.1)
    out.update(records=records, record_conf=rc[order])
    return out


@functools.lru_cache(maxsize=None)
def long_case(L):
    """M = 3 L + 70 fixed rows at D = 64; rows of L - 1, L, L + 1, 2 L, 3 L + 5 and 0 observations (L: the segment length)"""
    M, D = 3 * L + 70, 64
    rng = np.random.default_rng(91)
    F = rng.uniform(-0.5, 0.5, (M, D)).astype(np.float32)
    counts = [L - 1, L, L + 1, 2 * L, 3 * L + 5, 0]
    X0 = rng.uniform(-0.5, 0.5, (len(counts), D)).astype(np.float32)
    rows = [np.sort(rng.choice(M, n, replace=False)) for n in counts]
    ptr = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=ptr[1:])
    return _solved(F, X0, ptr, np.concatenate(rows).astype(np.int32), None, 3.0, 0.05, 0.1)


def interactions(nu=NU, ni=NI, seed=5, density=0.15):
    """a random interaction set with some repeated records -> structured array ('user_id', 'item_id')"""
    rng = np.random.default_rng(seed)
    u, i = np.nonzero(rng.random((nu, ni)) < density)
    u = np.concatenate([u, u[:7]]); i = np.concatenate([i, i[:7]])
    rec = np.zeros(u.size, dtype=[("user_id", np.int32), ("item_id", np.int32)])
    rec["user_id"], rec["item_id"] = u, i
    return rec


def csr_of(rec, n_rows, n_cols, rows="user_id", cols="item_id"):
    """the CSR ALSData must build from records: sorted, distinct -> (ptr, cols)"""
    key = np.unique(rec[rows].astype(np.int64) * n_cols + rec[cols])
    ptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(np.bincount(key // n_cols, minlength=n_rows), out=ptr[1:])
    return ptr, (key % n_cols).astype(np.int32)


# the block-diagonal toy set of the class test: 4 user groups x 4 item groups, users of group g like the items of group g
TOY = dict(groups=4, users_per=8, items_per=6, D=8, a=5.0, b=1.0, reg=3.0, sweeps=2, held=2, seed=0)


def toy_set():
    """-> (train records, held lists per user): every user trains on items_per - held items of its group; the `held` others of
    the group are what `recommend` must return first once the training items are excluded"""
    t = TOY
    rng = np.random.default_rng(11)
    us, its, held = [], [], []
    for u in range(t["groups"] * t["users_per"]):
        g = u // t["users_per"]
        own = g * t["items_per"] + rng.permutation(t["items_per"])
        held.append(np.sort(own[:t["held"]]))
        for i in own[t["held"]:]:
            us.append(u); its.append(i)
    rec = np.zeros(len(us), dtype=[("user_id", np.int32), ("item_id", np.int32)])
    rec["user_id"], rec["item_id"] = us, its
    return rec, held


def toy_init():
    """the tables the toy model starts from (Keras' uniform(-0.05, 0.05)) -> (U float32, V float32)"""
    t = TOY
    rng = np.random.default_rng(t["seed"])
    nu, ni = t["groups"] * t["users_per"], t["groups"] * t["items_per"]
    return (rng.uniform(-0.05, 0.05, (nu, t["D"])).astype(np.float32), rng.uniform(-0.05, 0.05, (ni, t["D"])).astype(np.float32))
