"""The seeded cases of the full-softmax step shared by tests/test_fullsoftmax_cpu.py (the reference, the headroom of the row-loss
bound, the launch geometry) and tests/test_gpu_fullsoftmax.py (the device against the float64 reference).

The four optimizers x with / without the bias table: each optimizer meets every shape once, under a different bias setting
than its neighbour meets it: 32 cases.  The shapes, (B, D, NU, NI, chunk_items, chunk_samples):
       1    4    40    40     0    0    a single sample
      15   24    50    63     0    0    one item short of a tile; D padded to 32
      17   64    30    65     0    0    one item and one sample past a tile
      65   64    30    40     0   64    more samples than items: every label repeats (n_j > 1); two sample chunks, the second one row
     130   50   200  3000   640   64    D no multiple of 4; five item chunks, the last ragged (3000 = 46 tiles + 56); three sample chunks
     300  128   500  5000  1024  128    five item chunks; three sample chunks
      64  256    60    80     0    0    the widest D
    1100   16  2000  2000     0    0    the launcher's own chunking, several workgroups on both sides
A chunk argument is the forced number of items / samples per chunk (a multiple of the tile width 64), 0 the launcher's own choice."""
import numpy as np

OPTS = ("sgd", "adagrad", "adam", "momentum")
LR = {"sgd": 0.05, "adagrad": 0.05, "adam": 0.002, "momentum": 0.05}
SCALE = 0.25                                  # tables uniform in (-SCALE, SCALE): scores of order 1 at D = 64

#          B     D    NU    NI  chunk_items  chunk_samples
SHAPES = ((1, 4, 40, 40, 0, 0),
          (15, 24, 50, 63, 0, 0),
          (17, 64, 30, 65, 0, 0),
          (65, 64, 30, 40, 0, 64),
          (130, 50, 200, 3000, 640, 64),
          (300, 128, 500, 5000, 1024, 128),
          (64, 256, 60, 80, 0, 0),
          (1100, 16, 2000, 2000, 0, 0))
# (item chunks, sample chunks) of the forced shapes
FORCED_CHUNKS = {3: (1, 2), 4: (5, 3), 5: (5, 3)}


def shape_case(si, opt="sgd", bias=True, seed=None):
    B, D, NU, NI, ci, cs = SHAPES[si]
    return dict(name=f"{opt}-{'b' if bias else 'nb'}-B{B}-D{D}-NI{NI}", opt=opt, bias=bias, B=B, D=D, NU=NU, NI=NI, chunk_items=ci,
                chunk_samples=cs, shape=si, seed=3000 + si if seed is None else seed)


def _cases():
    out = []
    for oi, opt in enumerate(OPTS):
        for si in range(len(SHAPES)):
            out.append(shape_case(si, opt, bias=(si + oi) % 2 == 0, seed=3000 + 8 * oi + si))
    return out


CASES = _cases()


def make(case, scale=SCALE):
    """-> U, V, b (float32; b None without the bias table), uid [B], pid [B] (int32)"""
    rng = np.random.default_rng(case["seed"])
    B, D, NU, NI = (case[k] for k in ("B", "D", "NU", "NI"))
    U = rng.uniform(-scale, scale, (NU, D)).astype(np.float32)
    V = rng.uniform(-scale, scale, (NI, D)).astype(np.float32)
    b = rng.uniform(-scale, scale, (NI, 1)).astype(np.float32)
    uid = rng.integers(0, NU, B).astype(np.int32)
    pid = rng.integers(0, NI, B).astype(np.int32)
    return U, V, (b if case["bias"] else None), uid, pid


def make_bags(case, max_len=6, empty=True):
    """ragged bags over the case's items -> ptr int32 [B + 1], items int32 [n]; bag 0 is empty where B > 1 and `empty`"""
    rng = np.random.default_rng(case["seed"] + 500)
    lens = rng.integers(1, max_len + 1, case["B"])
    if empty and case["B"] > 1:
        lens[0] = 0
    ptr = np.zeros(case["B"] + 1, np.int32)
    ptr[1:] = np.cumsum(lens)
    items = rng.integers(0, case["NI"], int(ptr[-1])).astype(np.int32)
    return ptr, items


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
