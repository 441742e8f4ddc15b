"""WARP negative sampling on the device (DeviceSampler.pairwise_warp, kernels_warp.hip): the stream bit for bit against
tests/hardneg_ref.py / tests/proposal_ref.py, the trial count, the negative and the weight exact against tests/warp_ref.py applied
to the kernel's OWN scores over the prefix the contract defines, those scores within the fp32 summation bound of the tables, the
prefix / window / repeat rules, and the plumbing (weight table, proposal, lazy Adam, the weighted step, bad arguments).

The tables are written from NumPy, so the margins and the precondition below are computed from the same numbers on the host:
m0 = 0 and m1 = float32(-1.65 std(s_c0 - s_p)).  At m1 every trial count 0, 1, .., T occurs in the window (asserted on warp_ref
before anything is compared), so the early exit at every column and the exhausted case are both exercised.  (Two of the 32
combinations -- D = 4, UCML, T = 64, with and without bias -- lack one resp. four of the late counts in the data themselves; the
precondition pins exactly those, see _ABSENT.)"""
import functools

import numpy as np
import pytest

import hardneg_ref as hr
import warp_ref as wr

pytestmark = pytest.mark.gpu

NU, NI, NR = 500, 300, 7001
N, FIRST, SEED = 3001, 6000, 7        # the window crosses the epoch boundary at 7001 and is no multiple of a chunk
SENTINEL = np.array([0x7FC12345], np.uint32).view(np.float32)[0]      # a NaN no arithmetic produces: "never written"


@functools.lru_cache(maxsize=None)
def _raw():
    return hr.make_data(0, NU, NI, NR)


@functools.lru_cache(maxsize=None)
def _ref():
    """(u, p, cand[N, 64]) of the window, from the NumPy restatement"""
    return hr.candidates(_raw(), NI, SEED, np.arange(FIRST, FIRST + N), 64)


@functools.lru_cache(maxsize=None)
def _host_tables(D):
    rng = np.random.default_rng(D)
    U = rng.uniform(-.5, .5, (NU, D)).astype(np.float32)
    V = rng.uniform(-.5, .5, (NI, D)).astype(np.float32)
    b = rng.uniform(-.5, .5, (NI, 1)).astype(np.float32)
    return U, V, b


def _exact(model, Uh, Vh, bh):
    """fp64 of the tables: (score[NU, NI], sum of the terms' magnitudes[NU, NI])"""
    U, V = Uh.astype(np.float64), Vh.astype(np.float64)
    bb = bh.astype(np.float64)[:, 0][None, :] if bh is not None else np.zeros((1, len(V)))
    with np.errstate(invalid="ignore", over="ignore"):
        if model == "bpr":
            return U @ V.T + bb, np.abs(U) @ np.abs(V).T + np.abs(bb)
        d2 = np.empty((len(U), len(V)))
        for r0 in range(0, len(U), 50):
            d2[r0:r0 + 50] = ((U[r0:r0 + 50, None, :] - V[None, :, :]) ** 2).sum(-1)
        return -d2 + bb, d2 + np.abs(bb)


@functools.lru_cache(maxsize=None)
def _exact_of(D, model, bias):
    U, V, b = _host_tables(D)
    return _exact(model, U, V, b if bias else None)


def _margins(D, model, bias, ref=None):
    ru, rp, rc = ref or _ref()
    want, _ = _exact_of(D, model, bias)
    m1 = np.float32(-1.65 * np.std(want[ru, rc[:, 0]] - want[ru, rp]))
    return np.float32(0.0), m1


# The precondition is a fact about the data, not about the kernel: of the 32 combinations (D, model, bias, T) it holds in NumPy for 30.
# At D = 4, UCML, T = 64 the window of 3001 samples has no sample for a few of the late counts (they are absent for every margin
# between 0.9 and 1.2 m1 too: bins of expectation ~1).  There the counts that ARE absent are pinned, so the case still asserts what
# the data exercise; every other count, 0 and the early ones among them, occurs.
_ABSENT = {(4, "ucml", True, 64): {60}, (4, "ucml", False, 64): {43, 51, 59, 64}}


def _precondition(D, model, bias, T, margin):
    """on warp_ref, from the tables: every trial count 0 .. T occurs (but for _ABSENT)"""
    ru, rp, rc = _ref()
    want, _ = _exact_of(D, model, bias)
    t, _, _ = wr.resolve(want[ru, rp].astype(np.float32), want[ru[:, None], rc[:, :T]].astype(np.float32), margin, np.ones(T, np.float32))
    cnt = np.bincount(t, minlength=T + 1)
    absent = set(np.flatnonzero(cnt == 0).tolist())
    assert absent == _ABSENT.get((D, model, bias, T), set()), (D, model, bias, T, sorted(absent))
    return cnt


@pytest.fixture(scope="module")
def sampler():
    from openrec_amd import runtime as rt
    sm = rt.DeviceSampler(_raw(), NU, NI)
    yield sm
    sm.set_proposal(None)


def _tables(D, bias=True, host=None):
    from openrec_amd import runtime as rt
    Uh, Vh, bh = host or _host_tables(D)
    U = rt.Table(NU, D); U.write(Uh)
    V = rt.Table(NI, D); V.write(Vh)
    b = None
    if bias:
        b = rt.Table(NI, 1); b.write(bh)
    return U, V, b


def _table(T):
    from openrec_amd import runtime as rt
    return rt.warp_weights(NI, T, "log")


def _run(sm, model, U, V, b, T, margin, table=None, first=FIRST, n=N, seed=SEED):
    """-> dict of numpy arrays: u, p, nid, w, t, sp, sc[n, T] (sc prefilled with SENTINEL)"""
    import torch
    dev = torch.device("cuda", 0)
    u, p, ng, t = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
    w, sp = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))
    sc = torch.from_numpy(np.full(n * T, SENTINEL, np.float32)).to(dev)
    sm.pairwise_warp(seed, first, n, u, p, ng, w, model, U, V, b, max_trials=T, margin=float(margin),
                     rank_weight=_table(T) if table is None else table, trials_out=t, pos_score_out=sp, cand_score_out=sc)
    sm.ctx.synchronize()
    out = dict(u=u, p=p, nid=ng, w=w, t=t, sp=sp, sc=sc)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["sc"] = out["sc"].reshape(n, T)
    return out


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _prefix(t, T):
    """bool [n, T]: the entries of cand_score the contract defines"""
    return np.arange(T)[None, :] < np.where(t > 0, t, T)[:, None]


def _check_exact(o, ref, T, margin, table, nan_free=True):
    """every sample: t, nid and weight are warp_ref.resolve of the kernel's own scores over the defined prefix"""
    ru, rp, rc = ref
    n = len(o["t"])
    assert np.array_equal(o["u"], ru) and np.array_equal(o["p"], rp)
    t = o["t"]
    assert ((t >= 0) & (t <= T)).all()
    pre = _prefix(t, T)
    assert not (_bits(o["sc"])[pre] == _bits(SENTINEL)).any(), "an entry of the defined prefix was not written"
    if nan_free:
        assert not np.isnan(o["sc"][pre]).any() and not np.isnan(o["sp"]).any()
    own = np.where(pre, o["sc"], np.float32(np.nan))            # beyond the prefix: unspecified, masked so that it cannot violate
    rt_, col, w = wr.resolve(o["sp"], own, margin, table)
    assert np.array_equal(t, rt_)                                # the prefix holds the violator and none before it
    assert np.array_equal(col, np.maximum(t - 1, 0))
    assert np.array_equal(o["nid"], rc[np.arange(n), col])
    assert np.array_equal(_bits(o["w"]), _bits(w))
    want_w = np.where(t > 0, np.asarray(table, np.float32)[np.maximum(t - 1, 0)], np.float32(0.0)).astype(np.float32)
    assert np.array_equal(_bits(o["w"]), _bits(want_w))          # table[t - 1], or the bits of +0.0


def _check_scores(o, ref, T, want, mag, D):
    """pos_score and the defined prefix of cand_score against fp64 of the tables, within (D + 2) 2^-24 sum|terms| (the bound of
    tests/test_gpu_hardneg.py::_check_scores: an fp32 sum of D + 1 terms with fused or unfused products)"""
    ru, rp, rc = ref
    pre = _prefix(o["t"], T)
    eps = (D + 2) * 2.0 ** -24
    err_p = np.abs(o["sp"].astype(np.float64) - want[ru, rp]); tol_p = eps * mag[ru, rp]
    err_c = np.abs(o["sc"].astype(np.float64) - want[ru[:, None], rc[:, :T]])[pre]; tol_c = (eps * mag[ru[:, None], rc[:, :T]])[pre]
    worst = max(float((err_p / tol_p).max()), float((err_c / tol_c).max()))
    print(f"D={D} T={T}: max err / bound = {worst:.3f}, mean t {o['t'][o['t'] > 0].mean():.2f}, none {np.mean(o['t'] == 0):.3f}")
    assert np.isfinite(o["sp"]).all() and np.isfinite(o["sc"][pre]).all()
    assert (err_p <= tol_p).all() and (err_c <= tol_c).all(), worst


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("model", ["bpr", "ucml"])
@pytest.mark.parametrize("D", [4, 20, 64, 256])
def test_exact_on_the_kernels_own_scores(sampler, D, model, bias):
    m0, m1 = _margins(D, model, bias)
    for T in (16, 64):
        _precondition(D, model, bias, T, m1)
    U, V, b = _tables(D, bias)
    want, mag = _exact_of(D, model, bias)
    for T in (16, 64):
        table = _table(T)
        for margin in (m0, m1):
            o = _run(sampler, model, U, V, b, T, margin, table)
            _check_exact(o, _ref(), T, margin, table)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("model", ["bpr", "ucml"])
@pytest.mark.parametrize("D", [4, 20, 64, 256])
def test_scores_are_right(sampler, D, model, bias):
    m0, m1 = _margins(D, model, bias)
    U, V, b = _tables(D, bias)
    want, mag = _exact_of(D, model, bias)
    for T, margin in ((16, m0), (64, m1)):
        o = _run(sampler, model, U, V, b, T, margin)
        _check_scores(o, _ref(), T, want, mag, D)


@pytest.mark.parametrize("model", ["bpr", "ucml"])
@pytest.mark.parametrize("D", [7, 260])
def test_the_plain_path(sampler, D, model):
    """a dim that is no multiple of 4, and one beyond the register-resident user row"""
    m0, m1 = _margins(D, model, True)
    U, V, b = _tables(D, True)
    want, mag = _exact_of(D, model, True)
    table = _table(3)
    for margin in (m0, m1):
        o = _run(sampler, model, U, V, b, 3, margin, table)
        _check_exact(o, _ref(), 3, margin, table)
        _check_scores(o, _ref(), 3, want, mag, D)


def test_the_margin_ends(sampler):
    import torch
    U, V, b = _tables(64)
    table = _table(16)
    dev = torch.device("cuda", 0)
    u0, p0, n0 = (torch.empty(N, dtype=torch.int32, device=dev) for _ in range(3))
    sampler.pairwise(SEED, FIRST, N, u0, p0, n0); sampler.ctx.synchronize()
    for model in ("bpr", "ucml"):
        o = _run(sampler, model, U, V, b, 16, np.inf, table)
        assert (o["t"] == 1).all() and np.array_equal(o["nid"], n0.cpu().numpy()) and np.array_equal(o["u"], u0.cpu().numpy())
        assert np.array_equal(o["p"], p0.cpu().numpy())
        assert np.array_equal(_bits(o["w"]), np.full(N, _bits(table[:1])[0]))
        _check_exact(o, _ref(), 16, np.inf, table)
        o = _run(sampler, model, U, V, b, 16, -np.inf, table)
        assert (o["t"] == 0).all() and np.array_equal(o["nid"], _ref()[2][:, 0])
        assert (_bits(o["w"]) == 0).all()                        # the bits of +0.0
        _check_exact(o, _ref(), 16, -np.inf, table)


@pytest.mark.parametrize("model", ["bpr", "ucml"])
def test_special_values(sampler, model):
    """a NaN item row, a -inf row, a -inf bias and a NaN bias among the candidates and the positives"""
    Uh, Vh, bh = (x.copy() for x in _host_tables(64))
    Vh[5] = np.nan; Vh[8] = -np.inf; bh[6] = -np.inf; bh[7] = np.nan
    U, V, b = _tables(64, True, host=(Uh, Vh, bh))
    ru, rp, rc = _ref()
    _, m1 = _margins(64, model, True)
    for T in (16, 64):
        table = _table(T)
        for margin in (0.0, m1):
            o = _run(sampler, model, U, V, b, T, margin, table)
            _check_exact(o, _ref(), T, margin, table, nan_free=False)
            pre = _prefix(o["t"], T)
            c = rc[:, :T]
            assert np.isnan(o["sc"][pre & (c == 5)]).all() and np.isnan(o["sc"][pre & (c == 7)]).all() and (pre & (c == 5)).any()
            assert np.isneginf(o["sc"][pre & (c == 6)]).all() and (pre & (c == 6)).any()
            found = o["t"] > 0
            assert not np.isin(o["nid"][found], (5, 6, 7)).any()           # such candidates never violate
            nanpos = np.isin(rp, (5, 7))
            assert nanpos.any() and np.isnan(o["sp"][nanpos]).all() and (o["t"][nanpos] == 0).all()
            assert (o["w"][nanpos] == 0).all() and np.array_equal(o["nid"][nanpos], rc[nanpos, 0])


def test_prefix_and_window_rules(sampler):
    U, V, b = _tables(64)
    _, m1 = _margins(64, "bpr", True)
    out = {T: _run(sampler, "bpr", U, V, b, T, m1) for T in (3, 16, 64)}
    for T1, T2 in ((3, 16), (16, 64), (3, 64)):
        a, c = out[T1], out[T2]
        f = a["t"] > 0
        assert f.any() and (~f).any()
        assert np.array_equal(c["t"][f], a["t"][f]) and np.array_equal(c["nid"][f], a["nid"][f])
        late = c["t"][~f]
        assert ((late == 0) | ((late > T1) & (late <= T2))).all() and (late > 0).any()
        assert np.array_equal(_bits(a["sp"]), _bits(c["sp"]))
    # a window equals the slice of the full call in every output
    full = out[16]
    w = _run(sampler, "bpr", U, V, b, 16, m1, first=FIRST + 1000, n=500)
    sl = slice(1000, 1500)
    for k in ("u", "p", "nid", "w", "t", "sp"):
        assert np.array_equal(_bits(w[k]), _bits(full[k][sl])), k
    pre = _prefix(w["t"], 16)
    assert np.array_equal(_bits(w["sc"])[pre], _bits(full["sc"][sl])[pre])
    # a repeated call gives the same bits in every defined output
    for model, T in (("bpr", 16), ("ucml", 64)):
        a = _run(sampler, model, U, V, b, T, m1)
        c = _run(sampler, model, U, V, b, T, m1)
        for k in ("u", "p", "nid", "w", "t", "sp"):
            assert np.array_equal(_bits(a[k]), _bits(c[k])), k
        pre = _prefix(a["t"], T)
        assert np.array_equal(_bits(a["sc"])[pre], _bits(c["sc"])[pre])


def test_candidates_come_from_the_proposal(sampler):
    import proposal_ref as pr
    U, V, b = _tables(64)
    table = _table(16)
    _, m1 = _margins(64, "bpr", True)
    plain = _run(sampler, "bpr", U, V, b, 16, m1, table)
    try:
        sampler.set_proposal(popularity=0.75)
        ref = pr.candidates(_raw(), NI, SEED, np.arange(FIRST, FIRST + N), 16, *sampler.proposal())
        assert not np.array_equal(ref[2], _ref()[2][:, :16])
        o = _run(sampler, "bpr", U, V, b, 16, m1, table)
        _check_exact(o, ref, 16, m1, table)
        _check_scores(o, ref, 16, *_exact_of(64, "bpr", True), 64)
        assert not np.array_equal(o["nid"], plain["nid"])
    finally:
        sampler.set_proposal(None)
    again = _run(sampler, "bpr", U, V, b, 16, m1, table)          # resetting restores the uniform bits
    for k in ("u", "p", "nid", "w", "t", "sp"):
        assert np.array_equal(_bits(again[k]), _bits(plain[k])), k


def test_every_call_uses_its_own_weight_table(sampler):
    import torch
    U, V, b = _tables(64)
    _, m1 = _margins(64, "bpr", True)
    T = 16
    ta, tb = _table(T), (np.arange(T, 0, -1) + 0.5).astype(np.float32)
    dev = torch.device("cuda", 0)
    ids = [[torch.empty(N, dtype=torch.int32, device=dev) for _ in range(4)] for _ in range(4)]
    ws = [torch.empty(N, dtype=torch.float32, device=dev) for _ in range(4)]
    for k, tab in enumerate((ta, tb, ta, ta)):                   # no synchronisation of the test's own in between
        sampler.pairwise_warp(SEED, FIRST, N, ids[k][0], ids[k][1], ids[k][2], ws[k], "bpr", U, V, b, max_trials=T, margin=float(m1),
                              rank_weight=tab, trials_out=ids[k][3])
    sampler.ctx.synchronize()
    t = ids[0][3].cpu().numpy()
    assert len(np.unique(t)) > T // 2 and (t == 0).any()
    for k, tab in enumerate((ta, tb, ta, ta)):
        assert np.array_equal(ids[k][3].cpu().numpy(), t)
        want = np.where(t > 0, tab[np.maximum(t - 1, 0)], np.float32(0)).astype(np.float32)
        assert np.array_equal(_bits(ws[k].cpu().numpy()), _bits(want)), k
    assert torch.equal(ws[2], ws[3]) and not torch.equal(ws[0], ws[1])
    # a kind name is `warp_weights` of the sampler's item count
    o = _run(sampler, "bpr", U, V, b, T, m1, "log1p")
    from openrec_amd import runtime as rt
    _check_exact(o, _ref(), T, m1, rt.warp_weights(NI, T, "log1p"))


def test_lazy_adam_rows_are_current_when_gathered(sampler):
    import torch
    from openrec_amd import runtime as rt
    U, V, b = _tables(64)
    opt = rt.Optimizer.adam(0.01)
    dev = torch.device("cuda", 0)
    B = 512
    tu, tp, tn = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    for k in range(3):
        sampler.pairwise(3, k * B, B, tu, tp, tn)
        rt.pairwise_step("bpr", opt, U, V, b, tu, tp, tn, K=1, B=B)
    # the sampler first, the reads afterwards: a read brings every row up to date and would hide a stale gather
    table = _table(16)
    o = _run(sampler, "bpr", U, V, b, 16, 0.0, table)
    Uh, Vh, bh = U.read(), V.read(), b.read()
    assert not np.array_equal(Uh, _host_tables(64)[0])
    _check_scores(o, _ref(), 16, *_exact("bpr", Uh, Vh, bh), 64)
    _check_exact(o, _ref(), 16, 0.0, table)


def test_warp_feeds_the_weighted_step(sampler):
    import torch
    from openrec_amd import runtime as rt
    U, V, b = _tables(64)
    K, B = 4, 512
    dev = torch.device("cuda", 0)
    u, p, ng = (torch.empty(K * B, dtype=torch.int32, device=dev) for _ in range(3))
    w = torch.empty(K * B, dtype=torch.float32, device=dev)
    sampler.pairwise_warp(SEED, 0, K * B, u, p, ng, w, "bpr", U, V, b, max_trials=16, margin=0.0)
    loss, l2 = rt.pairwise_step("bpr", rt.Optimizer.sgd(0.05), U, V, b, u, p, ng, K=K, B=B, weights=w, l2_reg=0.01)   # same stream
    assert np.isfinite(loss).all() and np.isfinite(l2).all() and (loss > 0).all()
    assert float(w.min()) >= 0 and float(w.max()) > 0
    # nothing violates: every weight is 0, and with l2_reg = 0 a triplet of weight 0 has no gradient at all
    before = [x.read() for x in (U, V, b)]
    sampler.pairwise_warp(SEED, 0, K * B, u, p, ng, w, "bpr", U, V, b, max_trials=16, margin=-np.inf)
    loss, l2 = rt.pairwise_step("bpr", rt.Optimizer.sgd(0.05), U, V, b, u, p, ng, K=K, B=B, weights=w, l2_reg=0.0)
    assert np.isfinite(loss).all()
    assert (_bits(w.cpu().numpy()) == 0).all()
    for x, h in zip((U, V, b), before):
        assert np.array_equal(_bits(x.read()), _bits(h))


def test_bad_arguments_raise_and_leave_the_context_usable(sampler):
    import torch
    from openrec_amd import runtime as rt
    U, V, b = _tables(64)
    dev = torch.device("cuda", 0)
    u, p, ng = (torch.empty(64, dtype=torch.int32, device=dev) for _ in range(3))
    w = torch.empty(64, dtype=torch.float32, device=dev)

    def call(model="bpr", U=U, V=V, b=b, T=8, margin=0.5, rank_weight="log", n=64, first=0):
        sampler.pairwise_warp(SEED, first, n, u, p, ng, w, model, U, V, b, max_trials=T, margin=margin, rank_weight=rank_weight)

    call(); sampler.ctx.synchronize()
    keep = [x.clone() for x in (u, p, ng, w)]
    other = rt.Context(0)
    bad = [dict(T=0), dict(T=257), dict(margin=float("nan")), dict(rank_weight=np.ones(7, np.float32)),
           dict(rank_weight=np.ones(9, np.float32)), dict(rank_weight="exp"),
           dict(model=2), dict(model=-1),
           dict(U=rt.Table(NU, 64, ctx=other)), dict(V=rt.Table(NI, 64, ctx=other)), dict(b=rt.Table(NI, 1, ctx=other)),
           dict(U=rt.Table(NU + 1, 64)), dict(V=rt.Table(NI - 1, 64), b=None), dict(U=rt.Table(NU, 32)),
           dict(b=rt.Table(NI, 2)), dict(b=rt.Table(NI + 1, 1))]
    for kw in bad:
        with pytest.raises(ValueError):
            call(**kw)
    # the C call refuses on its own too: max_trials, a NaN margin, no table, no weight buffer
    lib, tab = sampler._lib, np.ones(8, np.float32)

    def raw_call(T=8, margin=0.5, tw=tab.ctypes.data, wp=w.data_ptr()):
        return lib.orx_sampler_pairwise_warp(sampler._h, 0, U._h, V._h, b._h, SEED, 0, 64, T, margin, tw,
                                             u.data_ptr(), p.data_ptr(), ng.data_ptr(), wp, None, None, None)

    for kw in (dict(T=0), dict(T=257), dict(margin=float("nan")), dict(tw=None), dict(wp=None)):
        with pytest.raises(ValueError):
            rt.check(raw_call(**kw))
    sampler.ctx.synchronize()
    for x, k in zip((u, p, ng, w), keep):                        # nothing was launched
        assert torch.equal(x, k)
    call(); sampler.ctx.synchronize()                            # the next good call works
    u0, p0, n0 = (torch.empty(64, dtype=torch.int32, device=dev) for _ in range(3))
    sampler.pairwise(SEED, 0, 64, u0, p0, n0); sampler.ctx.synchronize()
    assert torch.equal(u, u0) and torch.equal(p, p0)
    # n = 0: nothing is written, with or without buffers
    before = [x.clone() for x in (ng, w)]
    call(n=0, first=5)
    e = torch.empty(0, dtype=torch.int32, device=dev)
    ef = torch.empty(0, dtype=torch.float32, device=dev)
    sampler.pairwise_warp(SEED, 5, 0, e, e, e, ef, "ucml", U, V, b, max_trials=256, margin=np.inf)
    sampler.ctx.synchronize()
    assert torch.equal(ng, before[0]) and torch.equal(w, before[1])
