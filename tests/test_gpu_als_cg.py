"""GPU: the conjugate-gradient ALS half-step (`rt.als_half_step(..., solver="cg")`, `rt.als_sweep`, `WRMF.fit_als`) and the
objective on the device (`rt.als_objective`) against tests/als_cg_ref.py.  The accuracy bound is relative to the float32 yardstick
of the SAME case and step count (tests/als_cg_cases.py; tests/test_als_cg_cpu.py shows it is non-zero, finite, and that another
float32 ordering stays within it): max|x - cg64| / max|cg64| <= FACTOR_CG e32cg, at up to 3 steps.  The objective is held to
(NU + NI + 2 D + 8) 2^-24 S.  Everything else is bit equality."""
import numpy as np
import pytest

import als_cases as ac
import als_cg_cases as cc
import als_cg_ref as cr
import als_ref as ar

pytestmark = pytest.mark.gpu


def _rt():
    from openrec_amd import runtime as rt
    return rt


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def _solve(rt, h, steps, device_csr=False, rows=None, X0=None, conf="own"):
    """the half's CG half-step on the device -> (x read back, the two tables)"""
    F = rt.Table(*h["F"].shape).write(h["F"])
    X = rt.Table(*h["X0"].shape).write(h["X0"] if X0 is None else X0)
    csr = rt.ALSCsr(h["ptr"], h["cols"], h["conf"] if isinstance(conf, str) else conf, h["F"].shape[0])
    if device_csr:
        csr = csr.to_device(F.ctx)
    rt.als_half_step(F, X, csr, h["a"], h["b"], h["reg"], rows=rows, solver="cg", cg_steps=steps)
    return X.read(), F, X


def _hold(what, x, h):
    err = ar.err_vs(x, h["x64"])
    print(f"{what}: err {err:.3g}, e32cg {h['e32cg']:.3g}, ratio {err / h['e32cg']:.3g}")
    assert np.isfinite(x).all(), what
    assert err <= cc.FACTOR_CG * h["e32cg"], (what, err, h["e32cg"])


# ---------------------------------------------------------------------------------------------- accuracy ---
@pytest.mark.parametrize("k", range(len(ac.ACC_CASES)), ids=lambda k: ac.case_id(ac.ACC_CASES[k]))
def test_accuracy_against_float64(k):
    rt = _rt()
    for side in ("user", "item"):
        for steps in cc.CG_STEPS:
            h = cc.solved(("acc", k, side), steps)
            x, F, X = _solve(rt, h, steps)
            _hold(f"{ac.case_id(ac.ACC_CASES[k])} {side} steps {steps}", x, h)
            assert np.array_equal(_bits(x[0]), np.zeros(x.shape[1], np.int32)), "the empty row is not all +0.0"
            assert np.array_equal(_bits(F.read()), _bits(h["F"])), "the fixed table changed"


def test_per_entry_confidence():
    rt = _rt()
    for steps in cc.CG_STEPS:
        h = cc.solved(("conf",), steps)
        x, _, _ = _solve(rt, h, steps)
        _hold(f"conf steps {steps}", x, h)


@pytest.mark.parametrize("which", cc.CONVERGED, ids=cc.half_id)
def test_many_steps_reach_the_direct_solution(which):
    """it is CG: on the well-conditioned halves at D = 8, 16 steps are the closed form"""
    rt = _rt()
    c = cc.converged(which)
    x, _, _ = _solve(rt, c, cc.CONVERGED_STEPS)
    err = ar.err_vs(x, c["x64"])
    print(f"err {err:.3g} against the direct float64 solution, yardstick {c['bound']:.3g}")
    assert np.isfinite(x).all() and err <= cc.FACTOR_CG * c["bound"]


def test_warm_start():
    """one step from two different starts: different rows, each within the bound of its own reference"""
    rt = _rt()
    k = next(i for i, c in enumerate(ac.ACC_CASES) if c["D"] == 50 and c["a"] == 41.0 and c["reg"] == 0.1)
    h = cc.solved(("acc", k, "user"), 1)
    x, _, _ = _solve(rt, h, 1)
    _hold("start X0", x, h)
    other = cc.solve(dict(cc.half(("acc", k, "user")), X0=np.ascontiguousarray(-h["X0"][::-1])), 1)
    y, _, _ = _solve(rt, other, 1)
    _hold("start -X0 reversed", y, other)
    assert np.abs(x[1:] - y[1:]).max() > 1e-3


def test_zero_residual_comes_back_as_zero():
    """conf all 0 with b = 0 and X0 = 0: y = 0, r = 0, and every row is exact +0.0 -- a 0 / 0 would show here"""
    rt = _rt()
    for D in (8, 64, 128):
        k = next(i for i, c in enumerate(ac.ACC_CASES) if c["D"] == D)
        h = dict(cc.half(("acc", k, "user")), b=0.0)
        x, _, _ = _solve(rt, h, 3, X0=np.zeros_like(h["X0"]), conf=np.zeros(h["cols"].size, np.float32))
        assert np.array_equal(_bits(x), np.zeros(x.shape, np.int32)), D


def test_a_equal_b_and_the_row_that_observes_everything():
    """a == b, conf NULL: every rank weight is zero and A v = b G v + reg v; row 4 of every case observes all M columns"""
    rt = _rt()
    k = next(i for i, c in enumerate(ac.ACC_CASES) if c["D"] == 50 and c["a"] == c["b"] and c["reg"] == 0.1)
    for steps in cc.CG_STEPS:
        h = cc.solved(("acc", k, "user"), steps)
        assert h["ptr"][5] - h["ptr"][4] == ac.NI
        x, _, _ = _solve(rt, h, steps)
        _hold(f"a == b, steps {steps}", x, h)
    k = next(i for i, c in enumerate(ac.ACC_CASES) if c["D"] == 128 and c["a"] == 41.0 and c["reg"] == 10.0)
    h = cc.solved(("acc", k, "item"), 3)
    x, _, _ = _solve(rt, h, 3)
    assert h["ptr"][5] - h["ptr"][4] == ac.NU
    _hold("D = 128, the row that observes all users in it", x, h)


# ------------------------------------------------------------------------------------------------- bits ---
def test_same_bits_however_the_rows_are_split():
    rt = _rt()
    k = next(i for i, c in enumerate(ac.ACC_CASES) if c["D"] == 64 and c["a"] == 41.0 and c["reg"] == 0.1)
    h = cc.half(("acc", k, "user"))
    R, steps = ac.NU, 3
    x, F, _ = _solve(rt, h, steps)
    assert np.array_equal(_bits(F.read()), _bits(h["F"])), "the fixed table changed"
    x2, _, _ = _solve(rt, h, steps)
    assert np.array_equal(_bits(x), _bits(x2)), "two calls differ"
    xd, _, _ = _solve(rt, h, steps, device_csr=True)
    assert np.array_equal(_bits(x), _bits(xd)), "host CSR and device CSR differ"
    for device_csr in (False, True):
        for reverse in (False, True):
            for chunk in (1, 5, R - 6):
                F = rt.Table(*h["F"].shape).write(h["F"]); X = rt.Table(*h["X0"].shape).write(h["X0"])
                csr = rt.ALSCsr(h["ptr"], h["cols"], None, ac.NI)
                if device_csr:
                    csr = csr.to_device(F.ctx)
                starts = list(range(0, R, chunk))
                for r0 in (reversed(starts) if reverse else starts):
                    rt.als_half_step(F, X, csr, h["a"], h["b"], h["reg"], rows=range(r0, min(r0 + chunk, R)), solver="cg", cg_steps=steps)
                assert np.array_equal(_bits(X.read()), _bits(x)), (device_csr, reverse, chunk)


def test_long_rows_and_every_break():
    rt = _rt()
    breaks = rt.als_cg_row_breaks(64)
    assert breaks == sorted(breaks) and len(breaks) >= 1
    L = rt.als_segment_len()
    h = cc.breaks_case(tuple(breaks), L)
    want = [L - 1, L, L + 1, 2 * L, 3 * L + 5, 0] + [n for t in breaks for n in (t - 1, t, t + 1)]
    assert list(np.diff(h["ptr"])) == want and h["F"].shape == (3 * L + 70, 64)
    R = len(want)
    x, F, _ = _solve(rt, h, 3)
    _hold("long rows", x, h)
    assert np.array_equal(_bits(x[5]), np.zeros(64, np.int32))
    assert np.array_equal(_bits(F.read()), _bits(h["F"])), "the fixed table changed"
    # a row is a function of its own data: alone in a call, on the device, in the whole call -- the same bits
    xd, _, _ = _solve(rt, h, 3, device_csr=True)
    assert np.array_equal(_bits(xd), _bits(x))
    for r in range(R):
        for device_csr in (False, True):
            xr, _, _ = _solve(rt, h, 3, rows=(r, 1), device_csr=device_csr)
            assert np.array_equal(_bits(xr[r]), _bits(x[r])), (r, device_csr)
            others = np.arange(R) != r
            assert np.array_equal(_bits(xr[others]), _bits(h["X0"][others])), "rows outside the range changed"


@pytest.mark.parametrize("slots", [0, 3, 5])
def test_long_rows_without_scratch_give_the_same_bits(slots, monkeypatch):
    """ORX_ALS_CG_SLOTS: with scratch for 0, 3 or 5 segments some or all of the long rows (2, 2, 2 and 4 segments) get none and are
    walked by a single wavefront"""
    rt = _rt()
    L = rt.als_segment_len()
    h = cc.breaks_case(tuple(rt.als_cg_row_breaks(64)), L)
    x, _, _ = _solve(rt, h, 3)
    for device_csr in (False, True):
        monkeypatch.setenv("ORX_ALS_CG_SLOTS", str(slots))
        xs, _, _ = _solve(rt, h, 3, device_csr=device_csr)
        monkeypatch.delenv("ORX_ALS_CG_SLOTS")
        assert np.array_equal(_bits(xs), _bits(x)), (slots, device_csr)


def test_breaks_of_every_dim():
    rt = _rt()
    for D in ac.DIMS + (1, 65):
        b = rt.als_cg_row_breaks(D)
        assert b == sorted(b) and all(t >= 1 for t in b), (D, b)
    assert rt.als_cg_row_breaks(0) == [] and rt.als_cg_row_breaks(129) == []


def test_the_cholesky_default_is_unchanged():
    rt = _rt()
    k = next(i for i, c in enumerate(ac.ACC_CASES) if c["D"] == 64 and c["a"] == 41.0 and c["reg"] == 0.1)
    h = ac.accuracy_case(k)["user"]
    out = []
    for kw in (dict(), dict(solver="cholesky"), dict(solver="cholesky", cg_steps=7)):
        F = rt.Table(*h["F"].shape).write(h["F"]); X = rt.Table(*h["X0"].shape).write(h["X0"])
        rt.als_half_step(F, X, rt.ALSCsr(h["ptr"], h["cols"], None, ac.NI), h["a"], h["b"], h["reg"], **kw)
        out.append(X.read())
    assert np.array_equal(_bits(out[0]), _bits(out[1])) and np.array_equal(_bits(out[0]), _bits(out[2]))
    assert ar.err_vs(out[0], h["x64"]) <= ac.FACTOR * h["e32"]
    x, _, _ = _solve(rt, h, 3)
    assert not np.array_equal(_bits(x), _bits(out[0])), "three CG steps are not the closed form"


# ------------------------------------------------------------------------------- descent and objective ---
@pytest.mark.parametrize("steps", [1, 3])
def test_three_sweeps_descend(steps):
    rt = _rt()
    d = cc.DESCENT
    a, b, reg = d["a"], d["b"], d["reg"]
    rec = ac.interactions()
    data = rt.ALSData(rec, ac.NU, ac.NI)
    pu, cu = ac.csr_of(rec, ac.NU, ac.NI)
    C, P = ar.dense_conf(pu, cu, None, a, b, (ac.NU, ac.NI))
    U0, V0 = ac.tables(d["D"], d["seed"])
    U = rt.Table(*U0.shape).write(U0); V = rt.Table(*V0.shape).write(V0)
    obj = [ar.objective(U0, V0, C, P, reg)]

    def look(what):
        Uh, Vh = U.read(), V.read()
        host, dev = ar.objective(Uh, Vh, C, P, reg), rt.als_objective(U, V, data, a, b, reg)
        bound = cr.objective_bound(Uh, Vh, pu, cu, None, a, b, reg)
        print(f"{what}: host {host:.12g}, device off by {abs(dev - host):.3g}, bound {bound:.3g}")
        assert abs(dev - host) <= bound, what
        obj.append(host)

    for s in range(d["sweeps"]):
        rt.als_half_step(V, U, data.by_user, a, b, reg, solver="cg", cg_steps=steps); look(f"sweep {s} user")
        rt.als_half_step(U, V, data.by_item, a, b, reg, solver="cg", cg_steps=steps); look(f"sweep {s} item")
    print(["%.9g" % o for o in obj])
    for o0, o1 in zip(obj, obj[1:]):
        assert o1 <= o0 + 1e-5 * abs(o0)
    assert obj[-1] < 0.5 * obj[0]


@pytest.mark.parametrize("case", cc.objective_cases(), ids=lambda c: c[0])
def test_objective_against_the_dense_float64(case):
    rt = _rt()
    name, U0, V0, ptr, cols, conf, a, b, reg = case
    C, P = ar.dense_conf(ptr, cols, conf, a, b, (ac.NU, ac.NI))
    dense, bound = ar.objective(U0, V0, C, P, reg), cr.objective_bound(U0, V0, ptr, cols, conf, a, b, reg)
    U = rt.Table(*U0.shape).write(U0); V = rt.Table(*V0.shape).write(V0)
    csr = rt.ALSCsr(ptr, cols, conf, ac.NI)
    got = rt.als_objective(U, V, csr, a, b, reg)
    print(f"{name}: dense {dense:.12g}, device off by {abs(got - dense):.3g}, bound {bound:.3g}")
    assert isinstance(got, float) and abs(got - dense) <= bound
    assert rt.als_objective(U, V, csr, a, b, reg) == got, "two calls differ"
    assert rt.als_objective(U, V, csr.to_device(U.ctx), a, b, reg) == got, "host CSR and device CSR differ"
    assert np.array_equal(_bits(U.read()), _bits(U0)) and np.array_equal(_bits(V.read()), _bits(V0))


def test_objective_of_non_finite_tables_and_bad_arguments():
    rt = _rt()
    name, U0, V0, ptr, cols, conf, a, b, reg = cc.objective_cases()[0]
    csr = rt.ALSCsr(ptr, cols, conf, ac.NI)
    Ub = U0.copy(); Ub[3, 1] = np.nan
    U = rt.Table(*U0.shape).write(Ub); V = rt.Table(*V0.shape).write(V0)
    assert not np.isfinite(rt.als_objective(U, V, csr, a, b, reg))
    cinf = np.full(cols.size, 2.0, np.float32); cinf[5] = np.inf
    U.write(U0)
    assert not np.isfinite(rt.als_objective(U, V, rt.ALSCsr(ptr, cols, cinf, ac.NI), a, b, reg))
    for kw in (dict(reg=0.0), dict(reg=float("nan")), dict(b=-1.0), dict(a=0.5, b=1.0)):
        with pytest.raises(ValueError):
            rt.als_objective(U, V, csr, **kw)
    with pytest.raises(ValueError):
        rt.als_objective(U, U, csr)
    with pytest.raises(ValueError):
        rt.als_objective(V, U, csr)                          # a CSR of another shape
    bad = cols.copy(); bad[2] = ac.NI
    with pytest.raises(IndexError):
        rt.als_objective(U, V, rt.ALSCsr(ptr, bad, None, ac.NI), a, b, reg)
    assert np.isfinite(rt.als_objective(U, V, csr, a, b, reg))      # the context stays usable


# ------------------------------------------------------------------------------------- through the class ---
def _toy_model(rt):
    from openrec_amd.tf2.recommenders import WRMF
    t = ac.TOY
    nu, ni = t["groups"] * t["users_per"], t["groups"] * t["items_per"]
    m = WRMF(t["D"], t["D"], nu, ni, a=t["a"], b=t["b"])
    U0, V0 = ac.toy_init()
    m.user_latent_factor.table.write(U0); m.item_latent_factor.table.write(V0)
    m.item_bias.table.fill(0.0)
    return m, nu, ni, U0, V0


def test_fit_als_with_cg_is_the_sweeps_and_recommends_the_held_items():
    rt = _rt()
    t, sweeps, steps = ac.TOY, cc.TOY_CG_SWEEPS, cc.TOY_CG_STEPS
    rec, held = ac.toy_set()
    m, nu, ni, U0, V0 = _toy_model(rt)
    for kw in (dict(solver="lu"), dict(solver="cg", cg_steps=0), dict(solver="cg", cg_steps=129)):
        with pytest.raises(ValueError):
            m.fit_als(rec, sweeps=sweeps, reg=t["reg"], **kw)
    assert np.array_equal(_bits(m.user_latent_factor.table.read()), _bits(U0))
    data = rt.ALSData(rec, nu, ni)
    o0 = m.als_objective(data, reg=t["reg"])
    assert m.fit_als(data, sweeps=sweeps, reg=t["reg"], solver="cg", cg_steps=steps) is m
    U = rt.Table(nu, t["D"]).write(U0); V = rt.Table(ni, t["D"]).write(V0)
    assert rt.als_objective(U, V, data, t["a"], t["b"], t["reg"]) == o0
    for _ in range(sweeps):
        rt.als_sweep(U, V, data, t["a"], t["b"], t["reg"], solver="cg", cg_steps=steps)
    assert np.array_equal(_bits(m.user_latent_factor.table.read()), _bits(U.read()))
    assert np.array_equal(_bits(m.item_latent_factor.table.read()), _bits(V.read()))
    o1 = m.als_objective(rec, reg=t["reg"])
    assert o1 == rt.als_objective(U, V, data, t["a"], t["b"], t["reg"]) and o1 < o0
    uid = np.arange(nu, dtype=np.int32)
    excl = rt.SparseMask(data.by_user.ptr, data.by_user.cols, ni)
    items, scores = m.recommend(uid, t["held"] + 1, excl)
    for u in range(nu):
        assert np.array_equal(np.sort(items[u, :t["held"]]), held[u]), (u, items[u], held[u])


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

    def raw(fixed, solved, a=1.0, b=1.0, reg=0.1, row0=0, nrows=ac.NU, flags=0, c=ctx, cg_steps=3):
        return lib.orx_als_half_step_cg(c._h, fixed._h, solved._h, h["ptr"].ctypes.data, h["cols"].ctypes.data, None, row0, nrows, a, b, reg,
                                        cg_steps, flags)

    bad = [dict(fixed=Fw, solved=X), dict(fixed=Fbig, solved=Xbig), dict(fixed=F, solved=X, reg=0.0), dict(fixed=F, solved=X, reg=-1.0),
           dict(fixed=F, solved=X, reg=nan), dict(fixed=F, solved=X, reg=inf), dict(fixed=F, solved=X, b=-0.5), dict(fixed=F, solved=X, a=0.5, b=1.0),
           dict(fixed=X, solved=X), dict(fixed=F2, solved=X), dict(fixed=F, solved=X, row0=-1), dict(fixed=F, solved=X, row0=1),
           dict(fixed=F, solved=X, row0=ac.NU + 1, nrows=0), dict(fixed=F, solved=X, nrows=-1), dict(fixed=F, solved=X, flags=2),
           dict(fixed=F, solved=X, cg_steps=0), dict(fixed=F, solved=X, cg_steps=-1), dict(fixed=F, solved=X, cg_steps=129)]
    for kw in bad:
        assert raw(**kw) == _ffi.ORX_ERR_ARG, kw
    for kw in bad:
        if "flags" in kw:
            continue
        kw = dict(kw)
        fixed, solved = kw.pop("fixed"), kw.pop("solved")
        row0, nrows = kw.pop("row0", 0), kw.pop("nrows", ac.NU)
        kw.setdefault("cg_steps", 3)
        use = csr if fixed.rows == ac.NI else rt.ALSCsr(h["ptr"], h["cols"], None, fixed.rows)
        with pytest.raises(ValueError):
            rt.als_half_step(fixed, solved, use, rows=(row0, nrows), solver="cg", **kw)
    for name in ("CG", "lu", None, ""):
        with pytest.raises(ValueError):
            rt.als_half_step(F, X, csr, solver=name)
        with pytest.raises(ValueError):
            rt.als_sweep(X, F, rt.ALSData(ac.interactions(), ac.NU, ac.NI, device=False), solver=name)
    with pytest.raises(ValueError):                        # cg_steps is checked whichever solver runs
        rt.als_half_step(F, X, csr, cg_steps=0)
    with pytest.raises(ValueError):                        # a CSR of another shape
        rt.als_half_step(F, X, rt.ALSCsr(h["ptr"][:-1], h["cols"][:h["ptr"][-2]], None, ac.NI), solver="cg")
    with pytest.raises(ValueError):
        rt.als_half_step(F, X, (h["ptr"], h["cols"]), solver="cg")
    ctx.synchronize()
    assert np.array_equal(_bits(X.read()), _bits(h["X0"])) and np.array_equal(_bits(F.read()), _bits(h["F"]))
    # nrows = 0 is a no-op, anywhere inside the table and at its end
    assert raw(F, X, row0=ac.NU, nrows=0) == _ffi.ORX_OK and raw(F, X, row0=3, nrows=0) == _ffi.ORX_OK
    rt.als_half_step(F, X, csr, rows=(5, 0), solver="cg")
    assert np.array_equal(_bits(X.read()), _bits(h["X0"]))


def test_column_out_of_range_raises_index_error():
    rt = _rt()
    h = cc.solved(("acc", 0, "user"), 3)
    F = rt.Table(*h["F"].shape).write(h["F"]); X = rt.Table(*h["X0"].shape).write(h["X0"])
    cols = h["cols"].copy()
    cols[h["ptr"][3]] = ac.NI                              # one past the fixed table's last row
    with pytest.raises(IndexError):
        rt.als_half_step(F, X, rt.ALSCsr(h["ptr"], cols, None, ac.NI), h["a"], h["b"], h["reg"], solver="cg")
    cols[h["ptr"][3]] = -1
    rt.als_half_step(F, X, rt.ALSCsr(h["ptr"], cols, None, ac.NI).to_device(F.ctx), h["a"], h["b"], h["reg"], solver="cg")
    with pytest.raises(IndexError):                        # a CSR on the device: no synchronisation in the call, the flag is asked for
        F.ctx.check_index_error()
    x, _, _ = _solve(rt, h, 3)                             # the context stays usable
    _hold("after the index errors", x, h)


def test_lazy_adam_tables_are_read_up_to_date():
    """after Adam steps applied lazily the CG half-step reads both tables -- the solved one is its warm start -- as an explicit
    read-back sees them, and leaves the solved table's optimizer slots alone"""
    rt = _rt()
    D = 64
    U0, V0 = ac.tables(D, 21)
    b0 = np.zeros((ac.NI, 1), np.float32)
    rng = np.random.default_rng(22)
    B = 16
    uid = rng.integers(0, ac.NU, B).astype(np.int32); iid = rng.integers(0, ac.NI, B).astype(np.int32)
    lab = (rng.random(B) < 0.5).astype(np.float32)
    data = rt.ALSData(ac.interactions(), ac.NU, ac.NI)

    def stepped():
        U = rt.Table(*U0.shape).write(U0); V = rt.Table(*V0.shape).write(V0); b = rt.Table(ac.NI, 1).write(b0)
        opt = rt.Optimizer.adam(0.01)
        for _ in range(2):
            rt.pointwise_step("wrmf", opt, U, V, b, None, uid, iid, lab, a=2.0, b_w=1.0)
        return U, V, opt

    U, V, opt = stepped()
    rt.als_half_step(V, U, data.by_user, 2.0, 1.0, 0.1, solver="cg", cg_steps=2)
    got = U.read()
    U2, V2, opt2 = stepped()
    Uh, Vh = U2.read(), V2.read()
    assert np.abs(Vh - V0).max() > 0 and np.abs(Uh - U0).max() > 0
    U3 = rt.Table(*U0.shape).write(Uh); V3 = rt.Table(*V0.shape).write(Vh)
    rt.als_half_step(V3, U3, data.by_user, 2.0, 1.0, 0.1, solver="cg", cg_steps=2)
    assert np.array_equal(_bits(got), _bits(U3.read()))
    assert np.array_equal(_bits(opt.slot(U, 0)), _bits(opt2.slot(U2, 0)))
