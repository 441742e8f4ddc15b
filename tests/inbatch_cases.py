"""The seeded cases of the in-batch step shared by tests/test_inbatch_cpu.py (the reference, the headroom of the row-loss bound,
the launch geometry) and tests/test_gpu_inbatch.py (the device against the float64 reference).

The four optimizers x with / without the bias table x K in {1, 3} x mask_hits on / off: 32 cases.  Each optimizer meets every
shape once, under a different (bias, K, mask) than the other optimizers meet it.  The shapes, (B, D, NU, NI, chunk):
    1    4   40   40   0    a single sample
    15   24   50   60   0    under one MFMA tile, D padded to 32
    17   64   30   40   0    one row past a tile of 16
    65   64   30   40   0    duplicate-heavy: 65 positives over 40 items, many hits; two tiles of 64
    130   50  200 3000  64   D no multiple of 4; three chunks, the last of them ragged (rows 128 .. 129)
    300  128  500 5000  64   five chunks, five row blocks
    64  256   60   80   0    the widest D, exact tiles
    1100   16 2000 2000   0    several workgroups per side at the launcher's own chunking
chunk is the forced number of columns per chunk (a multiple of the tile width 64), 0 the launcher's own choice."""
import numpy as np

OPTS = ("sgd", "adagrad", "adam", "momentum")
LR = {"sgd": 0.05, "adagrad": 0.05, "adam": 0.002, "momentum": 0.05}
SCALE = 0.25                                  # tables uniform in (-SCALE, SCALE): scores of order 1 at D = 64

#         B     D    NU    NI  chunk
SHAPES = ((1, 4, 40, 40, 0),
          (15, 24, 50, 60, 0),
          (17, 64, 30, 40, 0),
          (65, 64, 30, 40, 0),
          (130, 50, 200, 3000, 64),
          (300, 128, 500, 5000, 64),
          (64, 256, 60, 80, 0),
          (1100, 16, 2000, 2000, 0))
DUP_SHAPE = 3


def _cases():
    out = []
    for oi, opt in enumerate(OPTS):
        combos = [(bias, K, mask) for bias in (True, False) for K in (1, 3) for mask in (True, False)]
        for ci, (bias, K, mask) in enumerate(combos):
            si = (ci + 3 * oi + 2) % len(SHAPES)
            B, D, NU, NI, chunk = SHAPES[si]
            out.append(dict(name=f"{opt}-{'b' if bias else 'nb'}-K{K}-{'mask' if mask else 'nomask'}-B{B}-D{D}", opt=opt, bias=bias,
                            K=K, mask=mask, B=B, D=D, NU=NU, NI=NI, chunk=chunk, shape=si, seed=2000 + 8 * oi + ci))
    return out


CASES = _cases()


def make(case, scale=SCALE):
    """-> U, V, b (float32; b None without the bias table), uid [K, B], pid [K, B] (int32)"""
    rng = np.random.default_rng(case["seed"])
    K, B, D, NU, NI = (case[k] for k in ("K", "B", "D", "NU", "NI"))
    U = rng.uniform(-scale, scale, (NU, D)).astype(np.float32)
    V = rng.uniform(-scale, scale, (NI, D)).astype(np.float32)
    b = rng.uniform(-scale, scale, (NI, 1)).astype(np.float32)
    uid = rng.integers(0, NU, (K, B)).astype(np.int32)
    pid = rng.integers(0, NI, (K, B)).astype(np.int32)
    return U, V, (b if case["bias"] else None), uid, pid


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
