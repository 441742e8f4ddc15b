"""The fp16 MLP products (openrec_amd/csrc/kernels_gemm16.hip) one by one against exact references (tests/gemm16_ref.py), through the
diagnostic entry points of api_gemm16.hip.  The runners, the buffer layout, the guards and the operands' zero-padding contract are in
tests/gemm16_worker.py; the case tables below are data, and tests/test_gemm16_cpu.py proves from the launchers' own plan query that
they reach every form a shape can select on 256 CUs (and proves the exact regime exact).  The forms only the environment selects run
in one child process per setting (ENV_SETS).

A case row: id; the shape; regime "exact" (default: bit equality) or "round" (the derived element-wise bound); the epilogue."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

import gemm16_worker as W
from dlrm_util import record

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ nt, forward epilogue
# pad: lda = ldb = K rounded up to it (8: the TAIL forms unless K % 64 == 0; 64: the others); out: "C" / "C16" (the lean layers) / "both";
# ldc_extra / ldc16_extra: output leading dimension - N (default 4 / 8; 1 / 4: rows that are not 16-byte multiples -> element-wise stores)
NT_FWD = [
    dict(id="m1_n32_k8", M=1, N=32, K=8, out="both", bias=True, act=1),
    dict(id="m127_n40_k24", M=127, N=40, K=24, out="C", bias=True, act=0),
    dict(id="m128_n64_k64", M=128, N=64, K=64, out="both", bias=True, act=1, mask_out=True),
    dict(id="m128_n64_k72_pad64_nobias", M=128, N=64, K=72, pad=64, out="C16", act=0),
    dict(id="m129_n72_k72", M=129, N=72, K=72, out="both", bias=True, act=1, mask_out=True),
    dict(id="m333_n1000_k479", M=333, N=1000, K=479, out="both", bias=True, act=1, mask_out=True),
    dict(id="m333_n1024_k1024_c16", M=333, N=1024, K=1024, out="C16", bias=True, act=1, mask_out=True),
    dict(id="m333_n72_k24_pad64", M=333, N=72, K=24, pad=64, out="both", bias=False, act=1),
    dict(id="m256_n128_k8_oddld", M=256, N=128, K=8, out="both", bias=True, act=0, ldc_extra=1, ldc16_extra=4),
    dict(id="m8192_n1024_k64", M=8192, N=1024, K=64, out="both", bias=True, act=1, mask_out=True),
    dict(id="m8192_n1024_k1024", M=8192, N=1024, K=1024, out="C16", bias=True, act=1, mask_out=True),
    dict(id="m8229_n1000_k72", M=8192 + 37, N=1000, K=72, out="both", bias=True, act=1, mask_out=True),
    dict(id="m8229_n1024_k24_pad64", M=8192 + 37, N=1024, K=24, pad=64, out="C", bias=False, act=0),
    dict(id="m65573_n72_k24", M=65536 + 37, N=72, K=24, out="both", bias=True, act=1),
    dict(id="m65536_n40_k8_pad64", M=65536, N=40, K=8, pad=64, out="C16", bias=True, act=0),
    # rounding regime: each activation, with and without bias
    dict(id="r_m333_n1000_k479_sig", M=333, N=1000, K=479, regime="round", out="both", bias=True, act=2),
    dict(id="r_m129_n72_k1024_none", M=129, N=72, K=1024, regime="round", out="both", bias=False, act=0),
    dict(id="r_m8192_n1024_k1024_relu", M=8192, N=1024, K=1024, regime="round", out="both", bias=True, act=1),
    dict(id="r_m8229_n1000_k72_sig", M=8192 + 37, N=1000, K=72, regime="round", out="C16", bias=True, act=2),
    dict(id="r_m127_n40_k24_pad64_sig", M=127, N=40, K=24, pad=64, regime="round", out="C", bias=False, act=2),
]

# ------------------------------------------------------------------------------------------------ nt, backward epilogue
# y: where the layer below's output comes from -- "f32" (actY), "f16" (actY16), "mask" (mask_in written by a relu forward launch of the same
# [M][N]: must equal the actY16 form bit for bit); act_y 1 relu / 2 sigmoid; the exact regime's Y holds exact zeros (relu'(0) = 0)
NT_BWD = [
    dict(id="m1_n32_k8_f32_relu", M=1, N=32, K=8, y="f32", act_y=1, colsum=True),
    dict(id="m127_n40_k24_f16_sig", M=127, N=40, K=24, y="f16", act_y=2, colsum=True),
    dict(id="m129_n72_k72_f32_sig", M=129, N=72, K=72, y="f32", act_y=2, colsum=True, out="C"),
    dict(id="m333_n64_k64_pad64_f16_relu", M=333, N=64, K=64, pad=64, y="f16", act_y=1, colsum=True, out="C16"),
    dict(id="m333_n1000_k1024_mask", M=333, N=1000, K=1024, y="mask", act_y=1, colsum=True),
    dict(id="m128_n64_k479_mask", M=128, N=64, K=479, y="mask", act_y=1, colsum=True, out="C16"),
    dict(id="m8192_n1024_k64_mask", M=8192, N=1024, K=64, pad=64, y="mask", act_y=1, colsum=True, out="C16"),
    dict(id="m8229_n1000_k24_mask", M=8192 + 37, N=1000, K=24, y="mask", act_y=1, colsum=True),
    dict(id="m8192_n1024_k72_f16_sig", M=8192, N=1024, K=72, y="f16", act_y=2, colsum=True, out="C16"),
    dict(id="m8229_n1024_k8_pad64_f32_relu", M=8192 + 37, N=1024, K=8, pad=64, y="f32", act_y=1, colsum=True),
    dict(id="r_m333_n1000_k479_f16_sig", M=333, N=1000, K=479, regime="round", y="f16", act_y=2, colsum=True),
    dict(id="r_m8192_n1024_k1024_f16_relu", M=8192, N=1024, K=1024, regime="round", y="f16", act_y=1, colsum=True),
    dict(id="r_m129_n40_k72_f32_sig", M=129, N=40, K=72, regime="round", y="f32", act_y=2, colsum=True),
]

# ------------------------------------------------------------------------------------------------ tn (+ slab reduce)
# C[M][N] += scale * A[K][lda]^T B[K][ldb] from a non-zero C; lda / ldb default to M / N rounded up to 128; then: further batch sizes on the
# SAME slab workspace as the previous call left it (orx_gemm16_tn_form: "a later call with fewer samples must write the same S slices")
TN = [
    dict(id="t1_k8192", M=128, N=128, K=8192),                                   # 1 tile, S = 32, kchunk 256: no tail
    dict(id="t1_k64_then_1", M=128, N=128, K=64, then=(1,)),                     # 31 slices beyond the samples
    dict(id="t1_k2176_beyond_notail", M=128, N=128, K=2176),                     # kchunk 128: slices 17 .. 31 beyond the samples, no tail
    dict(id="t1_k6144_odd_steps", M=128, N=128, K=6144),                         # kchunk 192: three K steps per slice
    dict(id="t1_k4160_short_last", M=128, N=128, K=4160),                        # K % kchunk != 0
    dict(id="t1_edge_k333_scaled", M=100, N=72, K=333, lda=104, ldb=72, scale=1.0 / 1024),
    dict(id="t1_edge_k8192_notail", M=100, N=72, K=8192),                         # edge tile inside leading dimensions of 128: no tail
    dict(id="t1_edge_k63", M=13, N=128, K=63, lda=16, ldb=128),
    dict(id="t4_k4096_then_333", M=256, N=256, K=4096, then=(333, 128), scale=1.0 / 1024),     # 4 tiles, S = 32
    dict(id="t5_k4096", M=640, N=128, K=4096),                                   # 5 tiles, S = 16
    dict(id="t16_k65", M=512, N=512, K=65),                                      # 16 tiles, S = 16
    dict(id="t16_edge_k128", M=479, N=512, K=128, lda=480, ldb=512),             # lda < M rounded up to 128
    dict(id="t64_k8192", M=1024, N=1024, K=8192, scale=1.0 / 1024),              # 64 tiles, S = 4
    dict(id="t272_k128_s1", M=2048, N=2176, K=128),                              # 272 tiles: S = 1, C += in the kernel
    dict(id="t272_k64_s1_tail_scaled", M=2048, N=2176, K=64, scale=1.0 / 1024),
    dict(id="t289_edge_k65_s1", M=2048 + 37, N=2168, K=65, lda=2088, ldb=2168),
    dict(id="r_t1_k8192", M=128, N=128, K=8192, regime="round"),
    dict(id="r_t16_edge_k333", M=479, N=512, K=333, lda=480, ldb=512, regime="round", scale=1.0 / 1024),
    dict(id="r_t272_k128_s1", M=2048, N=2176, K=128, regime="round"),
]

# ------------------------------------------------------------------------------------------------ grouped launch
# a layer [B, out] -> [B, in]: X16 [B][ldx], dZ16 [B][lddz], W16 [nt_cols or in][ldw]; tails = (tn TAIL, nt TAIL) the row was written for
GROUP = [
    dict(id="g_ff", B=256, **{"in": 128}, out=128, ldx=128, lddz=128, ldw=128, tails=(0, 0)),
    dict(id="g_tf", B=333, **{"in": 128}, out=128, ldx=128, lddz=128, ldw=128, tails=(1, 0), act_y=2),
    dict(id="g_ft", B=256, **{"in": 128}, out=128, ldx=128, lddz=128, ldw=136, tails=(0, 1)),
    dict(id="g_tt", B=333, **{"in": 100}, out=72, ldx=104, lddz=72, ldw=72, tails=(1, 1), scale=1.0 / 1024),
    dict(id="g_ntcols", B=4096, **{"in": 479}, out=512, ldx=480, lddz=512, ldw=512, nt_cols=480, tails=(1, 0), y=False),
    dict(id="g_c5_512x256", B=8192, **{"in": 512}, out=256, ldx=512, lddz=256, ldw=256, tails=(0, 0), scale=1.0 / 1024),
    dict(id="r_g_tt", B=333, **{"in": 100}, out=72, ldx=104, lddz=72, ldw=72, tails=(1, 1), regime="round"),
    dict(id="r_g_c5_512x256", B=8192, **{"in": 512}, out=256, ldx=512, lddz=256, ldw=256, tails=(0, 0), regime="round"),
]

# ------------------------------------------------------------------------------------------------ the head
HEAD_FWD = [dict(id=f"b{B}_k{K}_act{a}{'_r' if r else ''}", B=B, K=K, act=a, regime="round" if r else "exact", pad=64 if K == 24 else 8)
            for (B, K, a, r) in [(1, 8, 0, 0), (255, 24, 1, 0), (256, 256, 0, 0), (257, 1000, 1, 0), (8192, 256, 1, 0), (8192, 1000, 0, 0),
                                 (257, 1000, 2, 1), (8192, 256, 2, 1), (255, 24, 0, 1), (1, 8, 1, 1)]]
HEAD_BWD = [dict(id=f"b{B}_k{K}_act{a}_below{b}", B=B, K=K, act=a, below=b)
            for (B, K, a, b) in [(1, 8, 0, 0), (255, 24, 1, 1), (256, 256, 2, 1), (257, 1000, 2, 2), (8192, 256, 2, 1), (8192, 1000, 0, 2),
                                 (257, 256, 1, 0), (256, 1000, 0, 1)]]
HEAD_BWD[3]["dz32"] = False

CAST = [dict(id="m333_n479", M=333, N=479, lds=479, ld16=480), dict(id="m7_n13_ld64", M=7, N=13, lds=16, ld16=64),
        dict(id="m4096_n1024", M=4096, N=1024, lds=1030, ld16=1024), dict(id="m1_n1", M=1, N=1, lds=1, ld16=8)]

# ------------------------------------------------------------------------------------------------ forms only the environment selects
# name -> (environment, [(kind, case)]); expect_form: what the plan query must report in THAT process (the case is void otherwise).
# Each set is one child process (the switches are read once per process).  The nt and tn switches are independent of each other.
_NT_SMALL = [dict(id="m333_n1000_k479", M=333, N=1000, K=479, out="both", bias=True, act=1),
             dict(id="m256_n128_k64_pad64", M=256, N=128, K=64, pad=64, out="both", bias=True, act=1),
             dict(id="m129_n72_k24_bwd", M=129, N=72, K=24, y="f16", act_y=2, colsum=True),
             dict(id="m512_n256_k128_bwd", M=512, N=256, K=128, pad=64, y="f16", act_y=1, colsum=True)]
_NT_BIG = [dict(id="m8229_n1000_k72", M=8192 + 37, N=1000, K=72, out="both", bias=True, act=1),
           dict(id="m8192_n1024_k128_bwd", M=8192, N=1024, K=128, pad=64, y="f16", act_y=1, colsum=True, out="C16")]
_TN_SET = [dict(id="t1_k8192", M=128, N=128, K=8192), dict(id="t1_edge_k333", M=100, N=72, K=333, lda=104, ldb=72, scale=1.0 / 1024),
           dict(id="t4_k4096_then_333", M=256, N=256, K=4096, then=(333,)), dict(id="t272_k128_s1", M=2048, N=2176, K=128),
           dict(id="t1_k2176_beyond", M=128, N=128, K=2176)]


def _with(cases, kind, **form):
    return [(kind, dict(c, expect_form=dict(form))) for c in cases]


ENV_SETS = {
    "tile2": ({"ORX_GEMM16_TILE": "2"}, _with(_NT_SMALL + _NT_BIG, "nt", cfg=2, stages=2)),
    "tile2_reg": ({"ORX_GEMM16_TILE": "2", "ORX_GEMM16_DMA": "0"}, _with(_NT_SMALL + _NT_BIG[:1], "nt", cfg=2, stages=0)),
    "tile1": ({"ORX_GEMM16_TILE": "1"}, _with(_NT_SMALL, "nt", cfg=1, stages=3)),
    "tile3": ({"ORX_GEMM16_TILE": "3"}, _with(_NT_BIG, "nt", cfg=3, stages=3)),
    "reg": ({"ORX_GEMM16_DMA": "0", "ORX_GEMM16_TN_DMA": "0"},
            _with(_NT_SMALL, "nt", cfg=3, stages=0) + _with(_NT_BIG, "nt", cfg=1, stages=0) + _with(_TN_SET, "tn", form=0)),
    "dma2": ({"ORX_GEMM16_DMA": "2", "ORX_GEMM16_TN_DMA": "2"},
             _with(_NT_SMALL, "nt", cfg=3, stages=2) + _with(_NT_BIG, "nt", cfg=1, stages=2) + _with(_TN_SET, "tn", form=2)),
    "wave128_tn3": ({"ORX_GEMM16_WAVE_TILE": "128", "ORX_GEMM16_TN_DMA": "3"},
                    _with(_NT_BIG, "nt", cfg=1, stages=3, wave_tile=128) + _with(_TN_SET, "tn", form=3)),
    "nts0": ({"ORX_GEMM16_NTS": "0", "ORX_GEMM16_NO_MASK": "1"},
             _with(_NT_SMALL[:2] + _NT_BIG, "nt", stages=3) + [("group", GROUP[3]), ("group", GROUP[0])]),
    "nts1": ({"ORX_GEMM16_NTS": "1"}, _with(_NT_SMALL[:2] + _NT_BIG, "nt", stages=3) + [("group", GROUP[3]), ("group", GROUP[0])]),
}
CHILD_TIMEOUT = 240          # seconds per child process


@pytest.fixture(scope="module")
def dev():
    d = W.Dev()
    yield d
    record("gemm16_kernel_tests", **d.stats)
    out = os.environ.get("ORX_GEMM16_STATS")          # worst error / bound per kernel, for profiles/gemm16_kernel_tests.txt
    if out:
        with open(out, "w") as f:
            json.dump(d.stats, f, indent=1, sort_keys=True)


def _ids(cases):
    return [c["id"] for c in cases]


@pytest.mark.parametrize("case", NT_FWD, ids=_ids(NT_FWD))
def test_nt_forward(dev, case):
    W.run_nt(dev, case)


@pytest.mark.parametrize("case", NT_BWD, ids=_ids(NT_BWD))
def test_nt_backward(dev, case):
    W.run_nt(dev, case)


@pytest.mark.parametrize("case", TN, ids=_ids(TN))
def test_tn(dev, case):
    W.run_tn(dev, case)


@pytest.mark.parametrize("case", GROUP, ids=_ids(GROUP))
def test_group(dev, case):
    W.run_group(dev, case)


@pytest.mark.parametrize("case", HEAD_FWD, ids=_ids(HEAD_FWD))
def test_head_forward(dev, case):
    W.run_head_fwd(dev, case)


@pytest.mark.parametrize("case", HEAD_BWD, ids=_ids(HEAD_BWD))
def test_head_backward(dev, case):
    W.run_head_bwd(dev, case)


@pytest.mark.parametrize("case", CAST, ids=_ids(CAST))
def test_cast16(dev, case):
    W.run_cast16(dev, case)


def test_refusals(dev):
    W.run_refusals(dev, masks_ok=True)


def test_device_has_the_cu_count_the_coverage_proof_assumes(dev):
    """tests/test_gemm16_cpu.py proves the tables' coverage for 256 CUs"""
    assert dev.num_cu == 256


def test_env_only_forms():
    """one fresh process per setting, each under its own timeout; the first child that fails or times out ends the test and nothing
    is started after it"""
    for name, (env, cases) in ENV_SETS.items():
        e = dict(os.environ)
        for k in list(e):
            if k.startswith("ORX_GEMM16_"):
                del e[k]
        e.update(env)
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gemm16_worker.py"), name], env=e, capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired as t:
            pytest.fail(f"{name} ({env}): no result after {CHILD_TIMEOUT} s; output so far:\n{t.stdout}\n{t.stderr}")
        assert r.returncode == 0 and f"DONE {len(cases)}" in r.stdout, f"{name} ({env}) failed (exit {r.returncode}):\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
