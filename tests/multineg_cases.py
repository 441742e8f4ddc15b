"""The seeded cases of the N-negative step shared by tests/test_multineg_cpu.py (headroom of the bounds, duplicate counts) and
tests/test_gpu_multineg.py (the device against the float64 reference).

Both losses x the four optimizers x with / without the bias table x K in {1, 3}: 32 cases.  Each optimizer meets every shape
once, under a different (loss, bias, K) than the other optimizers meet it.  The shapes cover B in {1, 7, 65, 300} (a partial
wavefront chunk, a ragged tail, more than one workgroup), N in {1, 2, 5, 16, 64}, tables of 30 to 5000 rows, and one D per
branch of the launcher's dispatch: 4 and 16 (four lanes per row), 24 (six lanes, rounded up to eight), 64, 128, 256, and the plain
path by both of its doors, 50 (no multiple of 4) and 260 (above 256).  Shape 0 is duplicate-heavy: 390 item references over 40
rows, 65 user references over 30."""
import numpy as np

OPTS = ("sgd", "adagrad", "adam", "momentum")
LR = {"sgd": 0.05, "adagrad": 0.05, "adam": 0.002, "momentum": 0.05}
SCALE = 0.25                                  # tables uniform in (-SCALE, SCALE): scores of order 1 at D = 64

#         B    N    D   NU    NI
SHAPES = ((65, 5, 64, 30, 40),
          (1, 1, 4, 40, 40),
          (7, 2, 24, 50, 60),
          (300, 16, 128, 500, 5000),
          (65, 64, 50, 200, 3000),
          (7, 16, 260, 60, 80),
          (300, 5, 16, 100, 2000),
          (7, 5, 256, 40, 50))


def _cases():
    out = []
    for oi, opt in enumerate(OPTS):
        combos = [(kind, bias, K) for kind in ("softmax", "logsig") for bias in (True, False) for K in (1, 3)]
        for ci, (kind, bias, K) in enumerate(combos):
            si = (ci + 3 * oi + 2) % len(SHAPES)
            B, N, D, NU, NI = SHAPES[si]
            out.append(dict(name=f"{kind}-{opt}-{'b' if bias else 'nb'}-K{K}-B{B}-N{N}-D{D}", kind=kind, opt=opt, bias=bias, K=K,
                            B=B, N=N, D=D, NU=NU, NI=NI, shape=si, seed=1000 + 8 * oi + ci))
    return out


CASES = _cases()


def make(case, scale=SCALE):
    """-> U, V, b (float32; b None without the bias table), uid [K, B], pid [K, B], nid [K, B, N] (int32)"""
    rng = np.random.default_rng(case["seed"])
    K, B, N, D, NU, NI = (case[k] for k in ("K", "B", "N", "D", "NU", "NI"))
    U = rng.uniform(-scale, scale, (NU, D)).astype(np.float32)
    V = rng.uniform(-scale, scale, (NI, D)).astype(np.float32)
    b = rng.uniform(-scale, scale, (NI, 1)).astype(np.float32)
    uid = rng.integers(0, NU, (K, B)).astype(np.int32)
    pid = rng.integers(0, NI, (K, B)).astype(np.int32)
    nid = rng.integers(0, NI, (K, B, N)).astype(np.int32)
    return U, V, (b if case["bias"] else None), uid, pid, nid


def make_opt(name):
    """the oracle's optimizer of a case (the device's takes the same constants)"""
    from oracle import numpy_oracle as orc
    from keras_momentum import Momentum
    lr = LR[name]
    if name == "sgd":
        return orc.SGD(lr)
    if name == "adagrad":
        return orc.Adagrad(lr)
    if name == "adam":
        return orc.AdamTFSparse(lr)
    return Momentum(lr, 0.9, True)
