"""The graphs and batches the LightGCN tests share (tests/test_lightgcn_cpu.py proves each case meaningful on the CPU,
tests/test_gpu_lightgcn.py holds the device to it).  References are computed once per process and never modified."""
import functools

import numpy as np

import lightgcn_ref as lr

LONG_NU, LONG_NI = 5000, 12


def int_tables(nu, ni, D, seed):
    """tables of integers in [-8, 8] as float32"""
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, (nu, D)).astype(np.float32), rng.integers(-8, 9, (ni, D)).astype(np.float32)


def long_degrees(S):
    return [0, 1, 63, 64, 65, S - 1, S, S + 1, 2 * S, 2 * S + 1, 4 * S + 1, LONG_NU]


@functools.lru_cache(maxsize=None)
def long_graph(S):
    """5000 users x 12 items; item i has long_degrees(S)[i] users, drawn without repetition -> (by_user, by_item)"""
    rng = np.random.default_rng(4242)
    us, its = [], []
    for i, n in enumerate(long_degrees(S)):
        us.append(rng.choice(LONG_NU, n, replace=False)); its.append(np.full(n, i))
    by_user, by_item = lr.csr_pair(np.concatenate(us), np.concatenate(its), LONG_NU, LONG_NI)
    assert list(np.diff(by_item[0])) == long_degrees(S)
    return by_user, by_item


@functools.lru_cache(maxsize=None)
def biregular():
    """64 users of degree 4, 16 items of degree 16: every edge of the symmetric normalisation weighs exactly 1/8"""
    u = np.repeat(np.arange(64), 4); i = (4 * u + np.tile(np.arange(4), 64)) % 16
    by_user, by_item = lr.csr_pair(u, i, 64, 16)
    assert set(np.diff(by_user[0])) == {4} and set(np.diff(by_item[0])) == {16}
    return by_user, by_item


GEN_NU, GEN_NI = 300, 200
GEN_EMPTY_USER = 17


@functools.lru_cache(maxsize=None)
def general_graph():
    """300 x 200, about 6000 records with Zipf items; user 17 and the items the draw never names are empty"""
    rng = np.random.default_rng(7)
    p = 1.0 / np.arange(1, GEN_NI - 9) ** 1.05            # the last 10 items are never drawn
    items = rng.choice(GEN_NI - 10, 6000, p=p / p.sum())
    users = rng.integers(0, GEN_NU, 6000)
    keep = users != GEN_EMPTY_USER
    by_user, by_item = lr.csr_pair(users[keep], items[keep], GEN_NU, GEN_NI)
    assert by_user[0][GEN_EMPTY_USER + 1] == by_user[0][GEN_EMPTY_USER] and (np.diff(by_item[0]) == 0).sum() >= 10
    return by_user, by_item


def float_tables(nu, ni, D, seed, scale=0.5):
    rng = np.random.default_rng(seed)
    return rng.uniform(-scale, scale, (nu, D)).astype(np.float32), rng.uniform(-scale, scale, (ni, D)).astype(np.float32)


def default_weights(L):
    return np.full(L + 1, np.float32(1) / np.float32(L + 1), np.float32)


GEN_CASES = [(D, L) for D in (16, 64) for L in (1, 3)]


@functools.lru_cache(maxsize=None)
def general_case(D, L):
    """-> dict: tables, graph, scales, the float64 propagation, the elementwise bound, the float32 yardstick's error"""
    by_user, by_item = general_graph()
    U, V = float_tables(GEN_NU, GEN_NI, D, 100 + D + L)
    su, sv = lr.scales(by_user[0]), lr.scales(by_item[0])
    al = default_weights(L)
    fu, fv = lr.propagate(U, V, by_user, by_item, su, sv, al)
    bu, bv, n_max = lr.bound(U, V, by_user, by_item, su, sv, al)
    return dict(U=U, V=V, by_user=by_user, by_item=by_item, su=su, sv=sv, al=al, fu=fu, fv=fv, bu=bu, bv=bv, n_max=n_max)


# ---- the step ---------------------------------------------------------------------------------------------------------------
STEP_D, STEP_L, STEP_B = 16, 2, 64


@functools.lru_cache(maxsize=None)
def step_batches(n=3):
    """n batches of 64 triplets over the general graph with repeated users and items; the empty user and the empty items -- rows
    with no path to any batch -- stay out of every batch"""
    rng = np.random.default_rng(99)
    out = []
    for _ in range(n):
        uid = rng.integers(0, 40, STEP_B); uid[uid == GEN_EMPTY_USER] = 3
        pid = rng.integers(0, 30, STEP_B); nid = rng.integers(0, 30, STEP_B)
        uid[1] = uid[0]; pid[3] = pid[2]; nid[5] = pid[2]
        out.append((uid.astype(np.int32), pid.astype(np.int32), nid.astype(np.int32)))
    return out


@functools.lru_cache(maxsize=None)
def step_setup():
    by_user, by_item = general_graph()
    U, V = float_tables(GEN_NU, GEN_NI, STEP_D, 555)
    su, sv = lr.scales(by_user[0]), lr.scales(by_item[0])
    al = default_weights(STEP_L)
    A = lr.dense_A(by_user, su, sv, GEN_NU, GEN_NI)
    return dict(U=U, V=V, by_user=by_user, by_item=by_item, su=su, sv=sv, al=al, A=A)


OPTS = {
    "sgd": (dict(kind="sgd", lr=1.0), ("sgd", dict(lr=1.0))),
    "momentum": (dict(kind="momentum", lr=0.5, momentum=0.9), ("momentum", dict(lr=0.5, momentum=0.9))),
    "nesterov": (dict(kind="momentum", lr=0.5, momentum=0.9, nesterov=True), ("momentum", dict(lr=0.5, momentum=0.9, nesterov=True))),
    "adagrad": (dict(kind="adagrad", lr=0.5, initial_accumulator_value=0.1, epsilon=1e-7), ("adagrad", dict(lr=0.5, initial_accumulator_value=0.1, epsilon=1e-7))),
    "adam": (dict(kind="adam", lr=0.002, beta_1=0.9, beta_2=0.999, epsilon=1e-7), ("adam", dict(lr=0.002, beta_1=0.9, beta_2=0.999, epsilon=1e-7))),
}


@functools.lru_cache(maxsize=None)
def step_ref(opt, steps, l2_reg, train_tables=("user", "item"), mixed=False):
    """the float64 result of `steps` graph steps (mixed: [graph, bpr, graph]) -> (U64, V64, [(loss, l2)])"""
    s = step_setup()
    bs = step_batches()
    seq = [("graph",) + bs[k] for k in range(steps)]
    if mixed:
        seq = [("graph",) + bs[0], ("bpr",) + bs[1], ("graph",) + bs[2]]
    return lr.train(s["A"], s["U"], s["V"], s["al"], lr.DenseOpt(**OPTS[opt][0]), seq, l2_reg, train_tables)


# ---- top-k ------------------------------------------------------------------------------------------------------------------
TOPK = dict(groups=4, users_per=8, items_per=6, D=8, k=3, L=2)


@functools.lru_cache(maxsize=None)
def topk_case():
    """a planted block graph; tables whose propagated scores are well separated -> dict with the float64 scores"""
    t = TOPK
    nu, ni = t["groups"] * t["users_per"], t["groups"] * t["items_per"]
    rng = np.random.default_rng(3)
    us, its = [], []
    for u in range(nu):
        g = u // t["users_per"]
        for i in g * t["items_per"] + rng.permutation(t["items_per"])[:4]:
            us.append(u); its.append(i)
    by_user, by_item = lr.csr_pair(us, its, nu, ni)
    U, V = float_tables(nu, ni, t["D"], 8, scale=1.0)
    su, sv = lr.scales(by_user[0]), lr.scales(by_item[0])
    al = default_weights(t["L"])
    fu, fv = lr.propagate(U, V, by_user, by_item, su, sv, al)
    bu, bv, _ = lr.bound(U, V, by_user, by_item, su, sv, al)
    S = fu @ fv.T
    sb = bu @ np.abs(fv).T + np.abs(fu) @ bv.T + bu @ bv.T          # what the tables' bounds allow a score to move
    order = np.argsort(-S, axis=1, kind="stable")
    top = np.take_along_axis(S, order, axis=1)
    gap = top[:, t["k"] - 1] - top[:, t["k"]]
    users = np.nonzero(gap > 100.0 * 2.0 * sb.max())[0].astype(np.int32)      # the k-th and (k+1)-th cannot change places
    return dict(U=U, V=V, by_user=by_user, by_item=by_item, su=su, sv=sv, al=al, fu=fu, fv=fv, bu=bu, bv=bv, nu=nu, ni=ni,
                users=users, items=order[users, :t["k"]], gap=gap, score_bound=float(sb.max()))
