"""GPU: alternating least squares for WRMF (`rt.als_half_step`, `rt.als_sweep`, `rt.ALSData`, `WRMF.fit_als`) against the float64
reference of tests/als_ref.py.  The accuracy bound is relative to the float32 yardstick of the SAME case (tests/als_cases.py;
tests/test_als_cpu.py shows it is non-zero and finite): max|x - x64| / max|x64| <= 4 e32.  Everything else is bit equality."""
import numpy as np
import pytest

import als_cases as ac
import als_ref as ar

pytestmark = pytest.mark.gpu


def _rt():
    from openrec_amd import runtime as rt
    return rt


def _solve(rt, h, device_csr=False, rows=None, conf=True):
    """the case's half-step on the device -> (x read back, the two tables)"""
    F = rt.Table(*h["F"].shape).write(h["F"])
    X = rt.Table(*h["X0"].shape).write(h["X0"])
    csr = rt.ALSCsr(h["ptr"], h["cols"], h["conf"] if conf else None, h["F"].shape[0])
    if device_csr:
        csr = csr.to_device(F.ctx)
    rt.als_half_step(F, X, csr, h["a"], h["b"], h["reg"], rows=rows)
    return X.read(), F, X


def _hold(what, x, h):
    err = ar.err_vs(x, h["x64"])
    print(f"{what}: err {err:.3g}, e32 {h['e32']:.3g}, ratio {err / h['e32']:.3g}")
    assert np.isfinite(x).all(), what
    assert err <= ac.FACTOR * h["e32"], (what, err, h["e32"])


# ---------------------------------------------------------------------------------------------- accuracy ---
@pytest.mark.parametrize("k", range(len(ac.ACC_CASES)), ids=lambda k: ac.case_id(ac.ACC_CASES[k]))
def test_accuracy_against_float64(k):
    rt = _rt()
    for side, h in ac.accuracy_case(k).items():
        x, F, X = _solve(rt, h)
        _hold(f"{ac.case_id(ac.ACC_CASES[k])} {side}", x, h)
        assert np.array_equal(x[0].view(np.int32), np.zeros(x.shape[1], np.int32)), "the empty row is not all +0.0"
        assert np.array_equal(F.read().view(np.int32), h["F"].view(np.int32)), "the fixed table changed"


def test_a_equal_b_gives_every_row_the_same_matrix():
    """a == b, conf NULL: c - b = 0, every rank update has weight zero and A_r = b G + reg I for all rows"""
    rt = _rt()
    k = next(i for i, c in enumerate(ac.ACC_CASES) if c["D"] == 50 and c["a"] == c["b"] and c["reg"] == 0.1)
    h = ac.accuracy_case(k)["user"]
    x, _, _ = _solve(rt, h)
    _hold("a == b", x, h)
    A = 1.0 * h["F"].astype(np.float64).T @ h["F"].astype(np.float64) + 0.1 * np.eye(50)
    y = np.stack([h["F"][h["cols"][h["ptr"][r]:h["ptr"][r + 1]]].astype(np.float64).sum(axis=0) for r in range(ac.NU)])
    assert ar.err_vs(x, np.linalg.solve(A, y.T).T) <= ac.FACTOR * h["e32"]


def test_per_entry_confidence_and_merged_duplicates():
    rt = _rt()
    h = ac.conf_case()
    x, _, _ = _solve(rt, h)
    _hold("conf, CSR given", x, h)
    # the same through ALSData: duplicates merged, their confidences summed
    data = rt.ALSData(h["records"], ac.NU, ac.NI, confidence=h["record_conf"])
    assert np.array_equal(data.by_user.ptr, h["ptr"]) and np.array_equal(data.by_user.cols, h["cols"])
    assert np.array_equal(data.by_user.conf, h["conf"]), "halves of a float32 add up exactly"
    assert data.by_item.cols.size == h["cols"].size and data.nnz == h["cols"].size
    F = rt.Table(*h["F"].shape).write(h["F"]); X = rt.Table(*h["X0"].shape).write(h["X0"])
    rt.als_half_step(F, X, data.by_user, h["a"], h["b"], h["reg"])
    assert np.array_equal(X.read().view(np.int32), x.view(np.int32))


def test_long_rows():
    rt = _rt()
    L = rt.als_segment_len()
    h = ac.long_case(L)
    assert list(np.diff(h["ptr"])) == [L - 1, L, L + 1, 2 * L, 3 * L + 5, 0] and h["F"].shape == (3 * L + 70, 64)
    x, _, _ = _solve(rt, h)
    _hold("long rows", x, h)
    assert not x[5].any()
    # a row is a function of its own data: alone in a call, on the device, in the whole call -- the same bits
    xd, _, _ = _solve(rt, h, device_csr=True)
    assert np.array_equal(xd.view(np.int32), x.view(np.int32))
    for r in range(6):
        xr, _, _ = _solve(rt, h, rows=(r, 1))
        assert np.array_equal(xr[r].view(np.int32), x[r].view(np.int32)), r
        others = np.arange(6) != r
        assert np.array_equal(xr[others].view(np.int32), h["X0"][others].view(np.int32)), "rows outside the range changed"


# ------------------------------------------------------------------------------------------- determinism ---
def test_same_bits_however_the_rows_are_split():
    rt = _rt()
    k = next(i for i, c in enumerate(ac.ACC_CASES) if c["D"] == 64 and c["a"] == 41.0 and c["reg"] == 0.1)
    h = ac.accuracy_case(k)["user"]
    R = ac.NU
    x, _, _ = _solve(rt, h)
    x2, _, _ = _solve(rt, h)
    assert np.array_equal(x.view(np.int32), x2.view(np.int32)), "two calls differ"
    xd, _, _ = _solve(rt, h, device_csr=True)
    assert np.array_equal(x.view(np.int32), xd.view(np.int32)), "host CSR and device CSR differ"
    for device_csr in (False, True):
        for reverse in (False, True):
            for chunk in (1, 5, R - 6):
                F = rt.Table(*h["F"].shape).write(h["F"]); X = rt.Table(*h["X0"].shape).write(h["X0"])
                csr = rt.ALSCsr(h["ptr"], h["cols"], None, ac.NI)
                if device_csr:
                    csr = csr.to_device(F.ctx)
                starts = list(range(0, R, chunk))
                for r0 in (reversed(starts) if reverse else starts):
                    rt.als_half_step(F, X, csr, h["a"], h["b"], h["reg"], rows=range(r0, min(r0 + chunk, R)))
                assert np.array_equal(X.read().view(np.int32), x.view(np.int32)), (device_csr, reverse, chunk)


# ----------------------------------------------------------------------------------------------- descent ---
def test_three_sweeps_descend():
    rt = _rt()
    a, b, reg = 41.0, 1.0, 0.1
    rec = ac.interactions()
    data = rt.ALSData(rec, ac.NU, ac.NI)
    pu, cu = ac.csr_of(rec, ac.NU, ac.NI)
    assert np.array_equal(data.by_user.ptr, pu) and np.array_equal(data.by_user.cols, cu)       # repeated records are one observation
    pi, ci = ac.csr_of(rec, ac.NI, ac.NU, "item_id", "user_id")
    assert np.array_equal(data.by_item.ptr, pi) and np.array_equal(data.by_item.cols, ci)
    C, P = ar.dense_conf(pu, cu, None, a, b, (ac.NU, ac.NI))
    U0, V0 = ac.tables(64, 4)
    U = rt.Table(*U0.shape).write(U0); V = rt.Table(*V0.shape).write(V0)
    obj = [ar.objective(U0, V0, C, P, reg)]
    for _ in range(3):
        rt.als_half_step(V, U, data.by_user, a, b, reg); obj.append(ar.objective(U.read(), V.read(), C, P, reg))
        rt.als_half_step(U, V, data.by_item, a, b, reg); obj.append(ar.objective(U.read(), V.read(), C, P, reg))
    print(["%.9g" % o for o in obj])
    for o0, o1 in zip(obj, obj[1:]):
        assert o1 <= o0 + 1e-5 * abs(o0)
    assert obj[-1] < 0.5 * obj[0]


# ------------------------------------------------------------------------------------- through the class ---
def _toy_model(rt):
    from openrec_amd.tf2.recommenders import WRMF
    t = ac.TOY
    nu, ni = t["groups"] * t["users_per"], t["groups"] * t["items_per"]
    m = WRMF(t["D"], t["D"], nu, ni, a=t["a"], b=t["b"])
    U0, V0 = ac.toy_init()
    m.user_latent_factor.table.write(U0); m.item_latent_factor.table.write(V0)
    return m, nu, ni, U0, V0


def test_fit_als_is_two_sweeps_and_recommends_the_held_items():
    rt = _rt()
    t = ac.TOY
    rec, held = ac.toy_set()
    m, nu, ni, U0, V0 = _toy_model(rt)
    with pytest.raises(ValueError):                       # Keras' uniform bias: ALS has no bias term
        m.fit_als(rec, sweeps=2, reg=t["reg"])
    assert np.array_equal(m.user_latent_factor.table.read().view(np.int32), U0.view(np.int32))
    m.item_bias.table.fill(0.0)
    assert m.fit_als(rec, sweeps=2, reg=t["reg"]) is m
    U = rt.Table(nu, t["D"]).write(U0); V = rt.Table(ni, t["D"]).write(V0)
    data = rt.ALSData(rec, nu, ni)
    for _ in range(2):
        rt.als_sweep(U, V, data, t["a"], t["b"], t["reg"])
    assert np.array_equal(m.user_latent_factor.table.read().view(np.int32), U.read().view(np.int32))
    assert np.array_equal(m.item_latent_factor.table.read().view(np.int32), V.read().view(np.int32))
    # an ALSData built once serves as well, and gives the same bits
    m2, *_ = _toy_model(rt)
    m2.item_bias.table.fill(0.0)
    m2.fit_als(data, sweeps=2, reg=t["reg"])
    assert np.array_equal(m2.item_latent_factor.table.read().view(np.int32), V.read().view(np.int32))
    with pytest.raises(ValueError):
        m2.fit_als(data, confidence=np.ones(rec.size))
    uid = np.arange(nu, dtype=np.int32)
    excl = rt.SparseMask(data.by_user.ptr, data.by_user.cols, ni)
    items, scores = m.recommend(uid, t["held"] + 1, excl)
    for u in range(nu):
        assert np.array_equal(np.sort(items[u, :t["held"]]), held[u]), (u, items[u], held[u])
        assert not np.isin(items[u], data.by_user.cols[data.by_user.ptr[u]:data.by_user.ptr[u + 1]]).any()


# --------------------------------------------------------------------------------------------- arguments ---
def test_bad_arguments_raise_before_any_launch():
    rt = _rt()
    from openrec_amd import _ffi
    lib = _ffi.load()
    h = ac.accuracy_case(0)["user"]                        # D = 8
    ctx = rt.default_context()
    F = rt.Table(*h["F"].shape).write(h["F"]); X = rt.Table(*h["X0"].shape).write(h["X0"])
    csr = rt.ALSCsr(h["ptr"], h["cols"], None, ac.NI)
    Fw = rt.Table(ac.NI, 12).fill(1.0)                     # another dim
    Fbig = rt.Table(ac.NI, 132).fill(1.0); Xbig = rt.Table(ac.NU, 132).fill(1.0)
    ctx2 = rt.Context(0)
    F2 = rt.Table(*h["F"].shape, ctx2).write(h["F"])
    nan, inf = float("nan"), float("inf")

    def raw(fixed, solved, a=1.0, b=1.0, reg=0.1, row0=0, nrows=ac.NU, flags=0, c=ctx):
        return lib.orx_als_half_step(c._h, fixed._h, solved._h, h["ptr"].ctypes.data, h["cols"].ctypes.data, None, row0, nrows, a, b, reg, flags)

    bad = [dict(fixed=Fw, solved=X), dict(fixed=Fbig, solved=Xbig), dict(fixed=F, solved=X, reg=0.0), dict(fixed=F, solved=X, reg=-1.0),
           dict(fixed=F, solved=X, reg=nan), dict(fixed=F, solved=X, reg=inf), dict(fixed=F, solved=X, b=-0.5), dict(fixed=F, solved=X, a=0.5, b=1.0),
           dict(fixed=X, solved=X), dict(fixed=F2, solved=X), dict(fixed=F, solved=X, row0=-1), dict(fixed=F, solved=X, row0=1),
           dict(fixed=F, solved=X, row0=ac.NU + 1, nrows=0), dict(fixed=F, solved=X, nrows=-1), dict(fixed=F, solved=X, flags=2)]
    for kw in bad:
        assert raw(**kw) == _ffi.ORX_ERR_ARG, kw
    for kw in bad:
        if "flags" in kw:
            continue
        kw = dict(kw)
        fixed, solved = kw.pop("fixed"), kw.pop("solved")
        row0, nrows = kw.pop("row0", 0), kw.pop("nrows", ac.NU)
        use = csr if fixed.rows == ac.NI else rt.ALSCsr(h["ptr"], h["cols"], None, fixed.rows)
        with pytest.raises(ValueError):
            rt.als_half_step(fixed, solved, use, rows=(row0, nrows), **kw)
    with pytest.raises(ValueError):                        # a CSR of another shape
        rt.als_half_step(F, X, rt.ALSCsr(h["ptr"][:-1], h["cols"][:h["ptr"][-2]], None, ac.NI))
    with pytest.raises(ValueError):
        rt.als_half_step(F, X, (h["ptr"], h["cols"]))
    ctx.synchronize()
    assert np.array_equal(X.read().view(np.int32), h["X0"].view(np.int32)) and np.array_equal(F.read().view(np.int32), h["F"].view(np.int32))
    # nrows = 0 is a no-op, anywhere inside the table and at its end
    assert raw(F, X, row0=ac.NU, nrows=0) == _ffi.ORX_OK and raw(F, X, row0=3, nrows=0) == _ffi.ORX_OK
    rt.als_half_step(F, X, csr, rows=(5, 0))
    assert np.array_equal(X.read().view(np.int32), h["X0"].view(np.int32))


def test_column_out_of_range_raises_index_error():
    rt = _rt()
    h = ac.accuracy_case(0)["user"]
    F = rt.Table(*h["F"].shape).write(h["F"]); X = rt.Table(*h["X0"].shape).write(h["X0"])
    cols = h["cols"].copy()
    cols[h["ptr"][3]] = ac.NI                              # one past the fixed table's last row
    csr = rt.ALSCsr(h["ptr"], cols, None, ac.NI)
    with pytest.raises(IndexError):
        rt.als_half_step(F, X, csr, h["a"], h["b"], h["reg"])
    cols[h["ptr"][3]] = -1
    rt.als_half_step(F, X, rt.ALSCsr(h["ptr"], cols, None, ac.NI).to_device(F.ctx), h["a"], h["b"], h["reg"])
    with pytest.raises(IndexError):                        # a CSR on the device: no synchronisation in the call, the flag is asked for
        F.ctx.check_index_error()
    # the context stays usable
    x, _, _ = _solve(rt, h)
    _hold("after the index errors", x, h)


def test_lazy_adam_tables_are_read_up_to_date():
    """after one Adam step (applied lazily: rows the batch did not touch still owe their decay step) the half-step reads the
    tables as an explicit read-back sees them"""
    rt = _rt()
    D = 64
    U0, V0 = ac.tables(D, 21)
    b0 = np.zeros((ac.NI, 1), np.float32)
    rng = np.random.default_rng(22)
    B = 16
    uid = rng.integers(0, ac.NU, B).astype(np.int32); iid = rng.integers(0, ac.NI, B).astype(np.int32)
    lab = (rng.random(B) < 0.5).astype(np.float32)
    rec = ac.interactions()
    data = rt.ALSData(rec, ac.NU, ac.NI)

    def stepped():
        U = rt.Table(*U0.shape).write(U0); V = rt.Table(*V0.shape).write(V0); b = rt.Table(ac.NI, 1).write(b0)
        opt = rt.Optimizer.adam(0.01)
        for _ in range(2):                                 # the second step leaves rows that owe a decay with non-zero moments
            rt.pointwise_step("wrmf", opt, U, V, b, None, uid, iid, lab, a=2.0, b_w=1.0)
        return U, V, opt

    U, V, opt = stepped()
    rt.als_half_step(V, U, data.by_user, 2.0, 1.0, 0.1)    # straight after the steps
    got = U.read()
    U2, V2, opt2 = stepped()
    Uh, Vh = U2.read(), V2.read()                          # explicit full read-back ...
    assert np.abs(Vh - V0).max() > 0
    U3 = rt.Table(*U0.shape).write(Uh); V3 = rt.Table(*V0.shape).write(Vh)      # ... and re-write
    rt.als_half_step(V3, U3, data.by_user, 2.0, 1.0, 0.1)
    assert np.array_equal(got.view(np.int32), U3.read().view(np.int32))
    # the optimizer slots of the solved table are left alone
    assert np.array_equal(opt.slot(U, 0).view(np.int32), opt2.slot(U2, 0).view(np.int32))
