"""Dynamic negative sampling on the device (DeviceSampler.pairwise_hard, kernels_hardneg.hip): the candidate stream bit for bit
against tests/hardneg_ref.py, the selection exact on the kernel's own scores, the scores within the fp32 summation bound of
the tables as read back (also after lazily-applied Adam steps), and the plumbing."""
import numpy as np
import pytest

import hardneg_ref as hr

pytestmark = pytest.mark.gpu

NU, NI, NR = 500, 300, 7001
N, FIRST, SEED = 3001, 6000, 7        # the window crosses the epoch boundary at 7001 and is no multiple of a block size


@pytest.fixture(scope="module")
def raw():
    return hr.make_data(0, NU, NI, NR)


@pytest.fixture(scope="module")
def ref(raw):
    """(u, p, cand[N, 64]) of the window, from the NumPy restatement"""
    return hr.candidates(raw, NI, SEED, np.arange(FIRST, FIRST + N), 64)


@pytest.fixture(scope="module")
def sampler(raw):
    from openrec_amd import runtime as rt
    return rt.DeviceSampler(raw, NU, NI)


def _tables(D, bias=True, seed=1):
    from openrec_amd import runtime as rt
    U = rt.Table(NU, D).init_uniform(-0.5, 0.5, seed=seed)
    V = rt.Table(NI, D).init_uniform(-0.5, 0.5, seed=seed + 1)
    b = rt.Table(NI, 1).init_uniform(-0.5, 0.5, seed=seed + 2) if bias else None
    return U, V, b


def _run(sm, model, U, V, b, M, first=FIRST, n=N, seed=SEED):
    """-> uid, pid, nid, cand[n, M], score[n, M] as numpy"""
    import torch
    dev = torch.device("cuda", 0)
    u, p, ng = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    c = torch.empty(n * M, dtype=torch.int32, device=dev)
    s = torch.empty(n * M, dtype=torch.float32, device=dev)
    sm.pairwise_hard(seed, first, n, u, p, ng, model, U, V, b, candidates=M, cand_out=c, cand_score_out=s)
    sm.ctx.synchronize()
    return u.cpu().numpy(), p.cpu().numpy(), ng.cpu().numpy(), c.cpu().numpy().reshape(n, M), s.cpu().numpy().reshape(n, M)


def _check_scores(model, Uh, Vh, bh, uid, cand, score):
    """every score against fp64 of the tables; the allowed difference is the bound of an fp32 sum of D + 1 terms with fused or
    unfused products, (D + 2) 2^-24 m with m the sum of the terms' magnitudes"""
    D = Uh.shape[1]
    u = Uh.astype(np.float64)[uid][:, None, :]
    v = Vh.astype(np.float64)[cand]
    bb = bh.astype(np.float64)[cand, 0] if bh is not None else 0.0
    if model == "bpr":
        want = (u * v).sum(-1) + bb
        m = np.abs(u * v).sum(-1) + np.abs(bb)
    else:
        want = -((u - v) ** 2).sum(-1) + bb
        m = ((u - v) ** 2).sum(-1) + np.abs(bb)
    err = np.abs(score.astype(np.float64) - want)
    tol = (D + 2) * 2.0 ** -24 * m
    worst = float((err / tol).max())
    print(f"{model} D={D} bias={bh is not None}: max err / bound = {worst:.3f}")
    assert np.isfinite(score).all() and (err <= tol).all(), worst


def _check_selection(nid, cand, score):
    j = hr.select(score)
    assert np.array_equal(nid, cand[np.arange(len(nid)), j])


def test_stream(sampler, ref):
    import torch
    U, V, b = _tables(64)
    ru, rp, rc = ref
    dev = torch.device("cuda", 0)
    u0, p0, n0 = (torch.empty(N, dtype=torch.int32, device=dev) for _ in range(3))
    sampler.pairwise(SEED, FIRST, N, u0, p0, n0); sampler.ctx.synchronize()
    u1, p1, n1, c1, _ = _run(sampler, "bpr", U, V, b, 1)
    assert np.array_equal(u1, u0.cpu().numpy()) and np.array_equal(p1, p0.cpu().numpy()) and np.array_equal(n1, n0.cpu().numpy())
    assert np.array_equal(c1[:, 0], n1)
    out = {}
    for M in (3, 8, 64):
        u, p, ng, c, _ = out[M] = _run(sampler, "bpr", U, V, b, M)
        assert np.array_equal(u, ru) and np.array_equal(p, rp)
        assert np.array_equal(c, rc[:, :M]), M
    assert np.array_equal(out[8][3][:, :3], out[3][3])
    w = _run(sampler, "bpr", U, V, b, 8, first=FIRST + 1000, n=500)
    for k in range(5):
        assert np.array_equal(w[k], out[8][k][1000:1500]), k


@pytest.mark.parametrize("model", ["bpr", "ucml"])
def test_selection_is_exact_on_the_kernels_own_scores(sampler, model):
    U, V, b = _tables(64)
    Vh = V.read()
    Vh[5] = np.nan; Vh[8] = -np.inf
    V.write(Vh)
    bh = b.read(); bh[6] = -np.inf; bh[7] = np.nan
    b.write(bh)
    for M in (8, 64):
        u, p, ng, c, s = _run(sampler, model, U, V, b, M)
        assert np.isnan(s[c == 5]).all() and np.isnan(s[c == 7]).all() and np.isneginf(s[c == 6]).all() and (c == 5).any()
        if model == "ucml":
            assert np.isneginf(s[c == 8]).all()
        _check_selection(ng, c, s)
        assert (ng != c[:, 0]).any()
    # a model that scores every candidate NaN keeps candidate 0, one that scores them equal too
    V.write(np.full((NI, 64), np.nan, np.float32))
    u, p, ng, c, s = _run(sampler, model, U, V, None, 8)
    assert np.isnan(s).all() and np.array_equal(ng, c[:, 0])
    V.fill(0.0)
    u, p, ng, c, s = _run(sampler, "bpr", U, V, None, 8)
    assert (s == 0).all() and np.array_equal(ng, c[:, 0])


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("model", ["bpr", "ucml"])
@pytest.mark.parametrize("D", [4, 20, 64, 256])
def test_scores_are_right(sampler, ref, D, model, bias):
    U, V, b = _tables(D, bias, seed=D)
    u, p, ng, c, s = _run(sampler, model, U, V, b, 8)
    assert np.array_equal(c, ref[2][:, :8])
    _check_scores(model, U.read(), V.read(), b.read() if bias else None, u, c, s)
    _check_selection(ng, c, s)


@pytest.mark.parametrize("model", ["bpr", "ucml"])
@pytest.mark.parametrize("D", [7, 260])
def test_scores_are_right_on_the_plain_path(sampler, ref, D, model):
    """a dim that is no multiple of 4, and one beyond the register-resident user row"""
    U, V, b = _tables(D, True, seed=D)
    u, p, ng, c, s = _run(sampler, model, U, V, b, 3)
    assert np.array_equal(c, ref[2][:, :3])
    _check_scores(model, U.read(), V.read(), b.read(), u, c, s)
    _check_selection(ng, c, s)


def test_lazy_adam_rows_are_current_when_gathered(sampler):
    import torch
    from openrec_amd import runtime as rt
    U, V, b = _tables(64, seed=40)
    opt = rt.Optimizer.adam(0.01)
    dev = torch.device("cuda", 0)
    B = 512
    tu, tp, tn = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    for k in range(3):
        sampler.pairwise(3, k * B, B, tu, tp, tn)
        rt.pairwise_step("bpr", opt, U, V, b, tu, tp, tn, K=1, B=B)
    # the sampler first, the read afterwards: a read brings every row up to date and would hide a stale gather
    u, p, ng, c, s = _run(sampler, "bpr", U, V, b, 8)
    _check_scores("bpr", U.read(), V.read(), b.read(), u, c, s)
    _check_selection(ng, c, s)


def test_bad_arguments_raise_and_leave_the_context_usable(sampler):
    import torch
    from openrec_amd import runtime as rt
    U, V, b = _tables(64)
    dev = torch.device("cuda", 0)
    u, p, ng = (torch.empty(64, dtype=torch.int32, device=dev) for _ in range(3))

    def call(model="bpr", U=U, V=V, b=b, M=8):
        sampler.pairwise_hard(SEED, 0, 64, u, p, ng, model, U, V, b, candidates=M)

    other = rt.Context(0)
    bad = [dict(M=0), dict(M=65), dict(model=2), dict(model=-1),
           dict(U=rt.Table(NU, 64, ctx=other)), dict(V=rt.Table(NI, 64, ctx=other)), dict(b=rt.Table(NI, 1, ctx=other)),
           dict(U=rt.Table(NU + 1, 64)), dict(V=rt.Table(NI - 1, 64), b=None), dict(U=rt.Table(NU, 32)),
           dict(b=rt.Table(NI, 2)), dict(b=rt.Table(NI + 1, 1))]
    for kw in bad:
        with pytest.raises(ValueError):
            call(**kw)
    call(); sampler.ctx.synchronize()
    u0, p0, n0 = (torch.empty(64, dtype=torch.int32, device=dev) for _ in range(3))
    sampler.pairwise(SEED, 0, 64, u0, p0, n0); sampler.ctx.synchronize()
    assert torch.equal(u, u0) and torch.equal(p, p0)
    # n = 0: nothing is written, with or without buffers
    before = ng.clone()
    sampler.pairwise_hard(SEED, 5, 0, u, p, ng, "bpr", U, V, b)
    e = torch.empty(0, dtype=torch.int32, device=dev)
    sampler.pairwise_hard(SEED, 5, 0, e, e, e, "ucml", U, V, b, candidates=64)
    sampler.ctx.synchronize()
    assert torch.equal(ng, before)


def test_a_repeated_call_gives_the_same_bits(sampler):
    U, V, b = _tables(64)
    for model, M in (("bpr", 8), ("ucml", 64)):
        a = _run(sampler, model, U, V, b, M)
        c = _run(sampler, model, U, V, b, M)
        for x, y in zip(a, c):
            assert np.array_equal(x.view(np.int32), y.view(np.int32))


def test_hard_negatives_feed_the_fused_step(sampler):
    import torch
    from openrec_amd import runtime as rt
    U, V, b = _tables(64)
    K, B = 4, 512
    dev = torch.device("cuda", 0)
    hard = [torch.empty(K * B, dtype=torch.int32, device=dev) for _ in range(3)]
    unif = [torch.empty(K * B, dtype=torch.int32, device=dev) for _ in range(3)]
    sampler.pairwise_hard(SEED, 0, K * B, *unif, "bpr", U, V, b, candidates=1)
    sampler.pairwise_hard(SEED, 0, K * B, *hard, "bpr", U, V, b, candidates=8)
    # forward only, on the same tables: a harder negative cannot lower the BPR loss of the same (u, p) in expectation
    l_unif, _ = rt.pairwise_loss("bpr", U, V, b, unif[0][:B], unif[1][:B], unif[2][:B])
    l_hard, _ = rt.pairwise_loss("bpr", U, V, b, hard[0][:B], hard[1][:B], hard[2][:B])
    assert np.isfinite(l_hard) and np.isfinite(l_unif) and l_hard > l_unif, (l_hard, l_unif)
    sampler.pairwise_hard(SEED, 0, K * B, *hard, "bpr", U, V, b, candidates=8)
    loss, l2 = rt.pairwise_step("bpr", rt.Optimizer.sgd(0.05), U, V, b, *hard, K=K, B=B)      # same stream: no sync in between
    assert np.isfinite(loss).all() and np.isfinite(l2).all()
    assert torch.equal(hard[0], unif[0]) and torch.equal(hard[1], unif[1]) and not torch.equal(hard[2], unif[2])
