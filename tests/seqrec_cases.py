"""The seeded cases of the history-pooled step shared by tests/test_seqrec_cpu.py (the reference against autograd, the headroom of
pool_bound) and tests/test_gpu_seqrec.py (the device against the float64 reference).

Tables of 40 to 300 items so that rows repeat; D in {1, 3, 64, 100, 256} (the plain walk by two doors, four rows per load, a
dim that fills 25 of 32 lanes, one row per load); B in {1, 7, 64, 300} (one bag, a partial workgroup, whole workgroups, many);
bag lengths drawn from {0, 1, 2, 4, 63, 64, 65, 130} (empty, shorter than a load round, one id fetch exactly, one more, three
fetches); N in {1, 16, 64}.  In every case item HOT sits in every non-empty bag and five times in bag 0 (which has 130 entries,
65 when B = 1), so its run in the sorted list crosses 64-entry blocks once B >= 64; bag 1 is one item repeated; pid and nid
are drawn from the items of the bags half of the time.  Each optimizer meets every pooling mode and both losses.

SGD with a bias table.  There the item table and the bias are applied as orx_multineg_step applies them: every occurrence is its
own fp32 read-modify-write (Keras' scatter-add), so a row with r occurrences is rounded r times in a step, while
conftest.delta_check allows steps + 1 roundings per element (its premise is one rounded update per step) and the float64
reference has none.  The one SGD case with a bias therefore has N = 1 over 300 items (two occurrences per row on average); the
duplicate-heavy item lists (1088 occurrences over 40 rows, 5100 over 150) go to the cases whose apply sums a row's occurrences
first -- SGD without a bias, and the other three optimizers either way.  The history table always takes the summing apply.

Adagrad and "sum" pooling.  With c_i = 1 the gradient rows of a 130-entry bag are 50 to 130 times those of the other modes, and so
is the fp32 error of the sum over the HOT row's occurrences, while the floor of delta_check (steps + 1 ulp of the table's
values) stays where it is and Adagrad's first step multiplies a gradient by lr / sqrt(0.1): at D = 64 a float32 NumPy run of
seqrec_ref itself sits at 0.96 to 1.15 of the bound.  Adagrad therefore meets "sum" at D = 1, B = 7.
tests/test_seqrec_cpu.py holds every case to that measure: a float32 run of the reference stays inside 0.6 of the bound."""
import numpy as np

OPTS = ("sgd", "adagrad", "adam", "momentum")
LENS = (0, 1, 2, 4, 63, 64, 65, 130)
HOT = 3
SCALE = 0.25
FIXED = ("fixed", 50)

#          D    B    N   NI   kind       opt         bias   pool    steps extras
_ROWS = ((64, 64, 16, 40, "softmax", "sgd", False, "mean", 1, True),
         (64, 300, 1, 300, "logsig", "adagrad", True, FIXED, 3, False),
         (100, 7, 64, 60, "softmax", "adam", True, FIXED, 1, False),
         (256, 64, 16, 120, "logsig", "momentum", False, "mean", 3, True),
         (1, 7, 1, 40, "softmax", "adagrad", True, "sum", 1, False),
         (3, 300, 1, 300, "logsig", "sgd", True, FIXED, 3, True),
         (64, 1, 64, 40, "softmax", "momentum", True, "sum", 1, False),
         (100, 64, 1, 300, "logsig", "adam", False, "mean", 3, False),
         (256, 7, 16, 50, "softmax", "sgd", False, FIXED, 1, False),
         (64, 300, 16, 100, "softmax", "adam", True, "sum", 3, True),
         (3, 64, 64, 80, "logsig", "momentum", True, "mean", 1, False),
         (1, 300, 16, 40, "softmax", "adagrad", False, FIXED, 1, False),
         (100, 300, 16, 150, "logsig", "sgd", False, "mean", 1, False),
         (64, 64, 16, 60, "logsig", "adagrad", True, "mean", 3, False),
         (256, 64, 1, 90, "softmax", "adam", False, "sum", 1, False),
         (64, 7, 16, 40, "softmax", "momentum", False, FIXED, 3, False))


def _pool_name(pool):
    return pool if isinstance(pool, str) else "fixed%g" % pool[1]


CASES = [dict(name=f"{kind}-{opt}-{'b' if bias else 'nb'}-{_pool_name(pool)}-D{D}-B{B}-N{N}-S{steps}", D=D, B=B, N=N, NI=NI, kind=kind,
              opt=opt, bias=bias, pool=pool, steps=steps, extras=extras, seed=2000 + i)
         for i, (D, B, N, NI, kind, opt, bias, pool, steps, extras) in enumerate(_ROWS)]


def make_bags(rng, B, NI):
    """-> ptr int32 [B + 1], items int32 [n]"""
    lens = rng.choice(LENS, B)
    lens[0] = 130 if B > 1 else 65
    if B > 1:
        lens[1] = 64
    if B > 2:
        lens[2] = 0
    bags = []
    for i, n in enumerate(lens):
        it = rng.integers(0, NI, n).astype(np.int32)
        if n:
            it[rng.integers(0, n)] = HOT
        bags.append(it)
    bags[0][[0, 17, 63, 64, 62 if B == 1 else 129]] = HOT
    if B > 1:
        bags[1][:] = 7
    ptr = np.zeros(B + 1, np.int32)
    ptr[1:] = np.cumsum(lens)
    return ptr, np.concatenate(bags).astype(np.int32)


def make_tables(case, scale=SCALE):
    """-> H, V, b (float32; b None without the bias table)"""
    rng = np.random.default_rng(case["seed"])
    NI, D = case["NI"], case["D"]
    H = rng.uniform(-scale, scale, (NI, D)).astype(np.float32)
    V = rng.uniform(-scale, scale, (NI, D)).astype(np.float32)
    b = rng.uniform(-scale, scale, (NI, 1)).astype(np.float32)
    return H, V, (b if case["bias"] else None)


def make_batches(case):
    """-> a list of case["steps"] batches dict(ptr, items, pid [B], nid [B, N], w [B] or None, off [B, N] or None)"""
    rng = np.random.default_rng(case["seed"] + 500)
    B, N, NI = case["B"], case["N"], case["NI"]
    out = []
    for _ in range(case["steps"]):
        ptr, items = make_bags(rng, B, NI)
        pid = rng.integers(0, NI, B).astype(np.int32)
        nid = rng.integers(0, NI, (B, N)).astype(np.int32)
        take = rng.random(B) < 0.5                      # ids that also occur in bags
        pid[take] = items[rng.integers(0, len(items), int(take.sum()))]
        nid[take, 0] = items[rng.integers(0, len(items), int(take.sum()))]
        w = off = None
        if case["extras"]:
            w = rng.uniform(0, 2, B).astype(np.float32)
            w[::5] = 0.0
            off = rng.normal(0, 1, (B, N)).astype(np.float32)
            if N > 1:
                off[:, 1] = -np.inf
        out.append(dict(ptr=ptr, items=items, pid=pid, nid=nid, w=w, off=off))
    return out
