"""The all-item scorer (runtime.score_all_items: score_mfma_kernel for D <= 256, score_all_kernel / score_all_nb_kernel beyond
and under ORX_SCORE_SIMPLE) element by element against tests/scorer_ref.py.

Top-K, the candidate scorer, the matrix-free metrics and the dense sampler routes are all held bit for bit to "what the scorer
returns", so this file holds the scorer to something that is not the scorer: a float64 reference with a derived per-element
fp32 bound (`check`), and small-integer tables whose result fp32 represents exactly in any summation order (`check_exact`).

Every call draws its tables from its own seed: the library's score scratch and torch's cached blocks are reused between calls,
and an element a kernel forgot to write must not be able to hold the right value from the call before."""
import numpy as np
import pytest

import scorer_ref as sr

pytestmark = pytest.mark.gpu

NU = 90
KINDS = sr.KINDS


def _rt():
    from openrec_amd import runtime as rt
    return rt


def _seed(*key):
    return np.random.default_rng([int(k) for k in key])


def _normal_tables(rng, NU, NI, D):
    U = rng.normal(size=(NU, D)).astype(np.float32); V = rng.normal(size=(NI, D)).astype(np.float32)
    w = rng.normal(size=(D, 1)).astype(np.float32); b = rng.normal(size=(NI, 1)).astype(np.float32)
    return U, V, w, b


def _uid(rng, nq, NU=NU):
    uid = rng.integers(0, NU, nq).astype(np.int32)
    uid[0] = NU - 1                              # the table's last row, and its first where there is room
    if nq > 2:
        uid[nq // 2] = 0
    return uid


def _score(kind, U, V, b, w, uid, device=False):
    """one scorer call on fresh tables"""
    rt = _rt()
    tU = rt.Table(*U.shape).write(U); tV = rt.Table(*V.shape).write(V)
    tb = None if b is None else rt.Table(V.shape[0], 1).write(b)
    tw = rt.Table(U.shape[1], 1).write(w) if kind == "gmf" else None
    return np.asarray(rt.score_all_items(kind, tU, tV, tb, uid, w=tw, device=device))


def _run(mode, kind, D, NI, nq, bias, key, what=""):
    """draw tables from `key`, score, hold the result to the reference in the given mode"""
    rng = _seed(*key)
    U, V, w, b = sr.exact_tables(rng, NU, NI, D) if mode == "exact" else _normal_tables(rng, NU, NI, D)
    uid = _uid(rng, nq)
    b = b if bias else None
    got = _score(kind, U, V, b, w, uid)
    what = "%s D=%d NI=%d nq=%d bias=%s %s" % (what, D, NI, nq, bias, mode)
    (sr.check_exact if mode == "exact" else sr.check)(got, kind, U, V, b, w, uid, what)


# ---- a. every dim route ----------------------------------------------------------------------------------------------------------
# matrix-core kernel: D = 16 KB exactly (16 .. 256), the float4 path with zero-filled columns (4, 12, 20, 24, 36, 100, 132, 200), the
# scalar path (1, 3, 17, 50, 127, 255) over all of KB = 1, 2, 4, 8, 16; the plain kernels (257, 300, and 1024 = 64 KB of dynamic LDS)
DIMS = (1, 3, 4, 12, 16, 17, 20, 24, 32, 36, 50, 64, 100, 127, 128, 132, 200, 255, 256, 257, 300, 1024)


@pytest.mark.parametrize("D", DIMS)
def test_every_dim_route(D):
    """nq = 70: two user-tile widths' worth (UW = 2; one 64-user group at KB = 16 plus a second blockIdx.y).  NI = 517: three runs
    of 256 items, the last of 5, and an odd row length, so every store is the scalar branch; NI = 516: 16-byte stores and a 4-item
    tail tile."""
    for NI in (517, 516):
        for ki, kind in enumerate(KINDS):
            for bias in (True, False):
                for mi, mode in enumerate(("exact", "bounded")):
                    _run(mode, kind, D, NI, 70, bias, (1, D, NI, ki, bias, mi))


def test_dim_beyond_the_lds_user_tile_is_refused():
    rt = _rt()
    tU = rt.Table(8, 1025); tV = rt.Table(9, 1025); tb = rt.Table(9, 1)
    for device in (False, True):
        with pytest.raises(ValueError, match="dim too large"):
            rt.score_all_items("dot", tU, tV, tb, np.zeros(3, np.int32), device=device)


# ---- b. shape edges --------------------------------------------------------------------------------------------------------------
EDGE_NI = (1, 3, 4, 63, 64, 65, 256, 257, 260)         # below one tile, one tile +- 1, one run (chunk = 256) + 1 / + 4
EDGE_NQ = (1, 17, 64, 65, 128, 129)                    # UW 1 | 2 at 64 | 65, a second blockIdx.y at 129 (65 at KB = 16)


@pytest.mark.parametrize("D", [20, 64, 255, 300])
def test_shape_edges(D):
    for ni, NI in enumerate(EDGE_NI):
        for nq in EDGE_NQ:
            for ki, kind in enumerate(("dot", "l2")):
                _run("exact", kind, D, NI, nq, True, (2, D, NI, nq, ki))
        nq = EDGE_NQ[ni % len(EDGE_NQ)]                # the diagonal of the grid in bounded mode
        for ki, kind in enumerate(("dot", "l2")):
            _run("bounded", kind, D, NI, nq, True, (3, D, NI, nq, ki))


# ---- c. long runs ----------------------------------------------------------------------------------------------------------------
def test_run_of_seven_tiles():
    """chunk = ceil(400003 * 1 / 1024) = 391 -> 448 items = 7 tiles of 64: above the minimum of 256, below the cap, and an odd
    tile count for the double buffer; the last run holds 400003 - 892 * 448 = 387 items (6 tiles and 3 items)"""
    for ki, kind in enumerate(KINDS):
        _run("exact", kind, 64, 400003, 3, True, (4, ki))


def test_run_at_the_cap():
    """chunk = ceil(4194309 / 1024) = 4097 -> 4160, capped at 4096 = 64 tiles; 1025 workgroups, the last with 5 items"""
    for ki, kind in enumerate(KINDS):
        _run("exact", kind, 4, 4096 * 1024 + 5, 2, True, (5, ki))


# ---- d. the plain kernels below 257 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [3, 64, 200])
def test_plain_kernels_as_ab_route(D, monkeypatch):
    """ORX_SCORE_SIMPLE (read per call) sends every dim to score_all_kernel / score_all_nb_kernel: 64 items x 16 users a block,
    so NI = 517 leaves 5 items and nq = 70 leaves 6 users in the last blocks"""
    monkeypatch.setenv("ORX_SCORE_SIMPLE", "1")
    for ki, kind in enumerate(KINDS):
        for bias in (True, False):
            for mi, mode in enumerate(("exact", "bounded")):
                _run(mode, kind, D, 517, 70, bias, (6, D, ki, bias, mi), what="plain")


# ---- e. position independence, bitwise -------------------------------------------------------------------------------------------
def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _same(a, c, what):
    assert np.array_equal(_bits(a), _bits(c)), what


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [24, 64, 255, 300])
def test_score_bits_do_not_depend_on_position(D, kind):
    """score(u, j) has one value, wherever j sits in the table or the tile (16-byte store or scalar tail), wherever u sits in the
    batch, however many users are scored with it (both user-tile widths) and whether V is scored whole or as a prefix: top-K scores
    its first P items as a problem of their own and the dense sampler routes score users in bounded batches.
    (This is the test that found the L2 norm sums compiled differently per user-tile width and per tile loop: at D = 24 the score
    of a user alone and of the same user among 129 differed in the last bit until the sums became explicit fmaf chains.  The
    period-7 table is scored under both widths for that reason.)"""
    rt = _rt()
    NI, NUe = 517, 140
    rng = _seed(7, D, KINDS.index(kind))
    U, V, w, b = _normal_tables(rng, NUe, NI, D)
    tU = rt.Table(NUe, D).write(U); tw = rt.Table(D, 1).write(w) if kind == "gmf" else None
    uid129 = rng.permutation(NUe)[:129].astype(np.int32)
    for p in (15, 16, 63, 64, 69):
        uid129[p] = uid129[0]
    uid70 = uid129[:70].copy()
    what = "D=%d %s" % (D, kind)

    def score(tV, tb, uid, **kw):
        return np.asarray(rt.score_all_items(kind, tU, tV, tb, uid, w=tw, **kw))

    # (the calls alternate between two tables, so that no call finds its own values left in the scratch by the one before)
    # users: one id at six places of the batch
    tV = rt.Table(NI, D).write(V); tb = rt.Table(NI, 1).write(b)
    S70 = score(tV, tb, uid70)
    sr.check(S70, kind, U, V, b, w, uid70, what + " nq=70")
    for p in (15, 16, 63, 64, 69):
        _same(S70[p], S70[0], what + ": row %d differs from row 0 of the same user" % p)
    # items: tables of period 7, under both user-tile widths (nq = 70 and 17)
    for n, first in ((70, 0), (17, 7)):
        idx = first + np.arange(NI) % 7
        Vp = V[idx]; bp = b[idx]
        S = score(rt.Table(NI, D).write(Vp), rt.Table(NI, 1).write(bp), uid70[:n])
        sr.check(S, kind, U, Vp, bp, w, uid70[:n], what + " periodic nq=%d" % n)
        _same(S, S[:, np.arange(NI) % 7], what + " nq=%d: an item's score depends on where it sits in the table" % n)
        if n == 70:
            # batch: alone, among 70, among 129
            S129 = score(tV, tb, uid129)
            sr.check(S129, kind, U, V, b, w, uid129, what + " nq=129")
            _same(S129[:70], S70, what + ": the first 70 of 129 users differ from the same 70 scored alone")
    for u in np.unique(uid129):
        one = score(tV, tb, np.array([u], np.int32))
        assert one.shape == (1, NI)
        for p in np.flatnonzero(uid129 == u):
            _same(S129[p], one[0], what + ": user %d alone differs from its row %d of 129" % (u, p))
    # prefix
    for P in (5, 64, 300):
        Sp = score(rt.Table(P, D).write(V[:P]), rt.Table(P, 1).write(b[:P]), uid70)
        _same(Sp, S70[:, :P], what + ": the first %d items scored as their own table differ" % P)


@pytest.mark.parametrize("D", [64, 300])
def test_host_and_device_output_are_equal(D):
    for ki, kind in enumerate(KINDS):
        rng = _seed(8, D, ki)
        U, V, w, b = _normal_tables(rng, NU, 517, D)
        uid = _uid(rng, 70)
        rt = _rt()
        tU = rt.Table(NU, D).write(U); tV = rt.Table(517, D).write(V); tb = rt.Table(517, 1).write(b)
        tw = rt.Table(D, 1).write(w) if kind == "gmf" else None
        host = rt.score_all_items(kind, tU, tV, tb, uid, w=tw)
        dev = np.asarray(rt.score_all_items(kind, tU, tV, tb, uid, w=tw, device=True))
        sr.check(host, kind, U, V, b, w, uid, "host D=%d" % D)
        assert dev.dtype == np.float32 and dev.shape == host.shape
        _same(dev, host, "D=%d %s: device output differs from the host output" % (D, kind))


# ---- f. non-finite confinement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [20, 64, 300])
def test_non_finite_values_stay_in_their_row_and_column(D, kind):
    """A NaN item row poisons its column, a NaN user row its row, a -inf bias its column, nothing else: the zero padding of the
    tiles (rows beyond nq and NI, columns beyond D) meets these values in the matrix product, and 0 * NaN must never reach a stored
    element.  For dot and GMF the -inf column is -inf; for L2 only "not finite" is asserted there -- the expanded form
    2 u.v - |u|^2 - |v|^2 + b may meet inf - inf, which is the kernel's business."""
    NI, nq = 517, 70
    j_nan, j_inf, q_nan = 100, 515, 37
    for bias in (True, False):
        rng = _seed(9, D, KINDS.index(kind), bias)
        U, V, w, b = _normal_tables(rng, NU, NI, D)
        uid = rng.permutation(NU)[:nq].astype(np.int32)          # distinct: the NaN user appears once
        V[j_nan] = np.nan
        U[uid[q_nan]] = np.nan
        b[j_inf] = -np.inf
        b = b if bias else None
        got = _score(kind, U, V, b, w, uid)
        # every element outside the poisoned row and columns within the bound, every element inside them non-finite
        sr.check(got, kind, U, V, b, w, uid, "D=%d bias=%s" % (D, bias))
        clean = np.ones((nq, NI), bool); clean[q_nan] = False; clean[:, j_nan] = False
        if bias:
            clean[:, j_inf] = False
        assert np.isfinite(got[clean]).all()
        assert np.isnan(got[:, j_nan]).all() and np.isnan(got[q_nan]).all()
        if bias:
            col = np.delete(got[:, j_inf], q_nan)
            assert not np.isfinite(col).any()
            if kind != "l2":
                assert (col == -np.inf).all()


# ---- g. L2 near zero distance ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128])
def test_l2_near_zero_distance(D, monkeypatch):
    """Rows of norm ~1 that are 1e-3 apart, and items that ARE a scored user's row (true score exactly b[j]).  The matrix-core
    route evaluates 2 u.v - |u|^2 - |v|^2, so its absolute error scales with |u|^2 + |v|^2 (a few ulp of 1, ~1e-7 here), NOT with
    the distance (~1e-6 * D): relative to the distance term the error is large, and a caller that ranks near-duplicates by L2 score
    sees fp32 noise of that size.  The bound of scorer_ref carries the same |u|^2 + |v|^2 and holds.  The plain route subtracts
    first, so there a copied row scores exactly b[j]."""
    NI, nq = 517, 70
    rng = _seed(10, D)
    off = rng.normal(size=D); off /= np.linalg.norm(off)
    U = (off + 1e-3 * rng.normal(size=(NU, D))).astype(np.float32)
    V = (off + 1e-3 * rng.normal(size=(NI, D))).astype(np.float32)
    b = rng.normal(size=(NI, 1)).astype(np.float32)
    uid = rng.permutation(NU)[:nq].astype(np.int32)
    copies = {3: 0, 64: 17, 255: 64, 256: 69, 516: 5}              # item j is the row of user uid[q]
    for j, q in copies.items():
        V[j] = U[uid[q]]
    ref = sr.reference("l2", U, V, b, None, uid)
    for j, q in copies.items():
        assert ref[q, j] == float(b[j, 0])
    got = _score("l2", U, V, b, None, uid)
    sr.check(got, "l2", U, V, b, None, uid, "D=%d" % D)
    monkeypatch.setenv("ORX_SCORE_SIMPLE", "1")
    plain = _score("l2", U, V, b, None, uid)
    sr.check(plain, "l2", U, V, b, None, uid, "plain D=%d" % D)
    for j, q in copies.items():
        assert plain[q, j] == b[j, 0]


# ---- h. ids ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,simple", [(64, False), (64, True), (300, False)])
def test_ids_outside_the_table_raise_and_leave_the_context_usable(D, simple, monkeypatch):
    """the kernels skip the load of a row that does not exist and raise a flag; the call reports it as IndexError"""
    if simple:
        monkeypatch.setenv("ORX_SCORE_SIMPLE", "1")
    rt = _rt()
    NI = 130
    for n, bad in enumerate((-1, NU)):
        rng = _seed(11, D, simple, n)
        U, V, w, b = _normal_tables(rng, NU, NI, D)
        tU = rt.Table(NU, D).write(U); tV = rt.Table(NI, D).write(V); tb = rt.Table(NI, 1).write(b)
        uid = _uid(rng, 20)
        wrong = uid.copy(); wrong[11] = bad
        for device in (False, True):
            with pytest.raises(IndexError):
                rt.score_all_items("dot", tU, tV, tb, wrong, device=device)
            got = rt.score_all_items("dot", tU, tV, tb, uid, device=device)          # the flag was cleared: the next call is clean
            sr.check(np.asarray(got), "dot", U, V, b, None, uid, "after id %d" % bad)
            uid = uid[::-1].copy()
        out = rt.score_all_items("dot", tU, tV, tb, np.zeros(0, np.int32))
        assert out.shape == (0, NI) and out.dtype == np.float32
