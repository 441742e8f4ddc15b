"""The seeded cases of the VBPR step shared by tests/test_vbpr_cpu.py (the two references, the float32 headroom) and
tests/test_gpu_vbpr.py (the device against the float64 reference).

The general case: NU = 300, NI = 400, Fd = 50, Dl = 12, Dc = 20, B = 192; tables and E uniform in +-0.05, F standard normal.  Fd and
Dc are no multiples of the K and N tiles (32 and 16), Fd is no multiple of 4 (the scalar staging path), B is three chunks of 64.
With far fewer items (NI = 48: about 8 occurrences per row) a float32 evaluation of the per-occurrence SGD adds itself leaves
conftest.delta_check on V, so the table sizes stay here.

The four optimizers x with / without the bias x with / without weights x K in {1, 3}: STEP_CASES takes each optimizer through
every (bias, weights) pair once and alternates K."""
import numpy as np

OPTS = ("sgd", "momentum", "adagrad", "adam")
LR = {"sgd": 0.05, "momentum": 0.05, "adagrad": 0.05, "adam": 0.002}
GENERAL = dict(NU=300, NI=400, Fd=50, Dl=12, Dc=20, B=192)
L2_REG, L2_PROJ = 0.01, 0.001
SCALE = 0.05


def _cases():
    out = []
    for oi, opt in enumerate(OPTS):
        for ci, (bias, wts) in enumerate(((True, True), (True, False), (False, True), (False, False))):
            K = 3 if (ci + oi) % 2 else 1
            out.append(dict(GENERAL, name=f"{opt}-{'b' if bias else 'nb'}-{'w' if wts else 'nw'}-K{K}", opt=opt, bias=bias, weights=wts,
                            K=K, seed=3000 + 4 * oi + ci))
    return out


STEP_CASES = _cases()


def make(case, K=None, scale=SCALE):
    """-> dict: U, V, b (None without the bias), E, F (float32), uid / pid / nid [K, B] (int32), w [K, B] float32 or None"""
    rng = np.random.default_rng(case.get("seed", 0))
    K = case.get("K", 1) if K is None else K
    NU, NI, Fd, Dl, Dc, B = (case[k] for k in ("NU", "NI", "Fd", "Dl", "Dc", "B"))
    U = rng.uniform(-scale, scale, (NU, Dl + Dc)).astype(np.float32)
    V = rng.uniform(-scale, scale, (NI, Dl)).astype(np.float32)
    b = rng.uniform(-scale, scale, (NI, 1)).astype(np.float32)
    E = rng.uniform(-scale, scale, (Fd, Dc)).astype(np.float32)
    F = rng.standard_normal((NI, Fd)).astype(np.float32)
    uid = rng.integers(0, NU, (K, B)).astype(np.int32)
    pid = rng.integers(0, NI, (K, B)).astype(np.int32)
    nid = rng.integers(0, NI, (K, B)).astype(np.int32)
    w = rng.uniform(0, 2, (K, B)).astype(np.float32)
    w[:, ::5] = 0.0                             # a weight of 0: the triplet keeps only its l2 part
    return dict(U=U, V=V, b=b if case.get("bias", True) else None, E=E, F=F, uid=uid, pid=pid, nid=nid,
                w=w if case.get("weights", False) else None)


def integer_features(rng, NI, Fd, Dc):
    """F with integers in [-4, 4], E with integers in [-8, 8] times 2^-6: every partial sum of F E is representable in fp32"""
    F = rng.integers(-4, 5, (NI, Fd)).astype(np.float32)
    E = (rng.integers(-8, 9, (Fd, Dc)) * 2.0 ** -6).astype(np.float32)
    return F, E
