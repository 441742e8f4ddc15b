"""What can be said about tests/test_gpu_gemm16.py without a device:

1. its exact regime is exact: for every exact case the float32 NumPy reference (NumPy's / BLAS's own summation order, FMA or not) equals
   the float64 one bit for bit -- every partial sum in every order is representable, so ANY correct fp32-accumulating kernel returns
   these bits;
2. its case tables reach every form of kernels_gemm16.hip that a SHAPE can select on 256 CUs, each with a tile that takes the fast
   (interior) epilogue and one that takes the element-wise (edge) one -- read from orx_gemm16_plan, the launchers' own code;
3. which forms only the environment selects, and that the child-process sets of the GPU module select them.

The 128 x 128 tile (cfg 2) is NOT reachable by shape: orx_gemm16_nt_plan takes it when blocks(128, 128) >= 2 cus while
blocks(256, 128) < cus, and ceil(M / 128) <= 2 ceil(M / 256) gives blocks(128, 128) <= 2 blocks(256, 128) < 2 cus for every M, N and
every CU count.  test_cfg2_is_unreachable_by_shape sweeps it as well.  It stays selectable by ORX_GEMM16_TILE=2 and is tested through the
child-process sets "tile2" (LDS-DMA) and "tile2_reg" (register-staged); DESIGN.md 7.2 says so."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import gemm16_ref as ref
import gemm16_worker as W
import test_gpu_gemm16 as T

CUS = 256


def _exact(cases):
    return [c for c in cases if c.get("regime", "exact") == "exact"]


def _same_bits(a32, a64, what):
    assert a32.dtype == np.float32 and a64.dtype == np.float64
    assert np.array_equal(a32.astype(np.float64), a64), f"{what}: the float32 and the float64 reference differ -- the case is not exact"
    assert np.abs(a64).max() < 2 ** 24


@pytest.mark.parametrize("case", _exact(T.NT_FWD + T.NT_BWD), ids=lambda c: c["id"])
def test_exact_regime_nt(case):
    h = W.nt_host(case)
    M, N = case["M"], case["N"]
    if case.get("y") == "mask":          # the device's relu forward of the layer below, which is exact too
        A2, B2 = W.mask_layer_host(M, N, "exact")
        y32, y64 = ref.nt(A2[:M], B2[:N], act=1, dtype=np.float32), ref.nt(A2[:M], B2[:N], act=1)
        _same_bits(y32, y64, case["id"] + " (mask forward)")
        h["Y"] = y64.astype(np.float16)
        assert np.array_equal(h["Y"].astype(np.float64), y64)
    v32, v64 = W.nt_reference(case, h, np.float32), W.nt_reference(case, h)
    _same_bits(v32, v64, case["id"])
    if case.get("colsum"):
        _same_bits(v32.sum(axis=0, dtype=np.float32), v64.sum(axis=0), case["id"] + " column sums")
    with np.errstate(over="ignore"):
        assert np.array_equal(v32.astype(np.float16), v64.astype(np.float16))


@pytest.mark.parametrize("case", _exact(T.TN), ids=lambda c: c["id"])
def test_exact_regime_tn(case):
    for K in [case["K"]] + list(case.get("then", ())):
        c = dict(case, K=K)
        h = W.tn_host(c)
        _same_bits(W.tn_reference(c, h, np.float32), W.tn_reference(c, h), f"{case['id']} K={K}")


@pytest.mark.parametrize("case", _exact(T.HEAD_FWD) + T.HEAD_BWD, ids=lambda c: c["id"])
def test_exact_regime_head(case):
    h = W.head_host(case)
    B, K = case["B"], case["K"]
    X, w = h["X"][:B, :K], h["w"][:K]
    if "below" in case:
        a, b = ref.head_bwd(X, w, h["dy"], h["pred"], case["act"], case["below"], np.float32), ref.head_bwd(X, w, h["dy"], h["pred"], case["act"], case["below"])
        for k in ("gW", "dZ", "gb_below"):
            _same_bits(a[k], b[k], f"{case['id']} {k}")
        assert float(a["gb"]) == float(b["gb"])
    else:
        _same_bits(ref.head_fwd(X, w, h["bias"], case["act"], np.float32), ref.head_fwd(X, w, h["bias"], case["act"]), case["id"])


# ------------------------------------------------------------------------------------------------ coverage, from the plan query
def _nt_paths(c, p):
    """which epilogues the case's tiles take: "fast" needs a tile inside the matrices and 16-byte rows everywhere (nt_epilogue_prefetch),
    "general" is every tile that reaches beyond M or N, and every tile when a row is not a 16-byte multiple or Y is fp32"""
    M, N = c["M"], c["N"]
    out = c.get("out", "both")
    rows16 = N % 8 == 0 and c.get("y") != "f32" and (out == "C16" or c.get("ldc_extra", 4) % 4 == 0) and (out == "C" or c.get("ldc16_extra", 8) % 8 == 0) \
        and (c.get("y") is None or c.get("ldy_extra", 8) % 8 == 0)
    paths = set()
    if rows16 and M >= p["bm"] and N >= p["bn"]:
        paths.add("fast")
    if not rows16 or M % p["bm"] or N % p["bn"]:
        paths.add("general")
    return paths


def _nt_forms(cases):
    hit = set()
    for c in cases:
        M, N, K, lda, ldb = W.nt_layout(c)
        p, _ = W.plan(CUS, M, N, K, lda, ldb)
        for path in _nt_paths(c, p):
            hit.add((p["cfg"], p["stages"], p["tail"], path))
    return hit


def _no_env():
    return not any(k.startswith("ORX_GEMM16_") for k in os.environ)


def test_cfg2_is_unreachable_by_shape():
    if not _no_env():
        pytest.skip("ORX_GEMM16_* set in this process")
    seen = set()
    for cus in (CUS, 304, 64, 1):
        for M in list(range(1, 600, 7)) + [2 ** k + d for k in range(7, 21) for d in (-1, 0, 1, 37)]:
            for N in (32, 40, 64, 72, 127, 128, 129, 255, 256, 257, 1000, 1024, 4096, 65536):
                p, _ = W.plan(cus, M, N, 64, 64, 64)
                seen.add(p["cfg"])
                assert p["stages"] == 3 and p["wave_tile"] == 64
    assert seen == {1, 3}


def test_tables_reach_every_nt_form_a_shape_selects():
    if not _no_env():
        pytest.skip("ORX_GEMM16_* set in this process")
    # by shape: the 256 x 128 and the 128 x 64 tile, three LDS-DMA stages, TAIL or not (leading dimensions % 64), fast or general epilogue
    reachable = {(cfg, 3, tail, path) for cfg in (1, 3) for tail in (0, 1) for path in ("fast", "general")}
    for name, cases in (("forward", T.NT_FWD), ("backward", T.NT_BWD)):
        hit = _nt_forms(cases)
        assert hit <= reachable, f"{name}: the plan reports forms this test does not know: {hit - reachable}"
        assert hit == reachable, f"{name}: no case for {sorted(reachable - hit)}"
    # the backward table: every source of Y with both activations' worth, and masks in both configurations
    ys = {(c["y"], c["act_y"]) for c in T.NT_BWD}
    assert {("f32", 1), ("f32", 2), ("f16", 1), ("f16", 2), ("mask", 1)} <= ys
    assert {W.plan(CUS, c["M"], c["N"], c["K"], 64, 64)[0]["cfg"] for c in T.NT_BWD if c["y"] == "mask"} == {1, 3}
    # the issue's minimum sets
    for key, need in (("M", {1, 127, 128, 129, 333, 8192, 8192 + 37}), ("N", {32, 40, 64, 72, 1000, 1024}), ("K", {8, 24, 64, 72, 479, 1024})):
        assert need <= {c[key] for c in T.NT_FWD}, key
    assert {c.get("pad", 8) for c in T.NT_FWD} == {8, 64} and {c.get("out", "both") for c in T.NT_FWD} == {"C", "C16", "both"}
    assert {c.get("act", 0) for c in T.NT_FWD} == {0, 1, 2} and {bool(c.get("bias")) for c in T.NT_FWD} == {True, False}


def test_tables_reach_every_tn_form_a_shape_selects():
    if not _no_env():
        pytest.skip("ORX_GEMM16_* set in this process")
    hit, S_seen = set(), set()
    for c in T.TN:
        for K in [c["K"]] + list(c.get("then", ())):
            _, p = W.plan(CUS, c["M"], c["N"], K, c.get("lda", W.up(c["M"], 128)), c.get("ldb", W.up(c["N"], 128)))
            assert p["form"] == 4                                   # by shape: always the two-K-group kernel
            edge = bool(c["M"] % 128 or c["N"] % 128)
            hit.add((p["tail"], "edge" if edge else "interior", "split" if p["S"] > 1 else "direct"))
            S_seen.add(p["S"])
            nk = (min(K, p["kchunk"]) + 63) // 64
            if K % p["kchunk"]:
                hit.add("short last slice")
            if nk % 2:
                hit.add("odd K steps")
            if (K + p["kchunk"] - 1) // p["kchunk"] < p["S"]:
                hit.add(("slices beyond the samples", p["tail"]))
    want = {(t, e, s) for t in (0, 1) for e in ("edge", "interior") for s in ("split", "direct")} - {(0, "edge", "direct")}
    # ((0, "edge", "direct"): an edge tile without a tail needs leading dimensions beyond M / N at >= 257 tiles -- same code as the split form's)
    assert want <= hit, sorted(want - {h for h in hit if isinstance(h, tuple) and len(h) == 3})
    assert {"short last slice", "odd K steps", ("slices beyond the samples", 0), ("slices beyond the samples", 1)} <= hit
    assert {32, 16, 1} <= S_seen and len(S_seen - {32, 16, 1}) >= 1
    assert {1, 63, 64, 65, 128, 333, 4096, 8192} <= {K for c in T.TN for K in [c["K"]] + list(c.get("then", ()))}
    assert {c.get("scale", 1.0) for c in T.TN} == {1.0, 1.0 / 1024}


def test_tables_reach_every_group_form():
    if not _no_env():
        pytest.skip("ORX_GEMM16_* set in this process")
    tails, grouped = set(), set()
    for c in T.GROUP:
        g = W.group_plan(CUS, c["B"], c["in"], c["out"], c["ldx"], c["lddz"], c["ldw"], c.get("nt_cols", 0))
        assert (g["tn_tail"], g["nt_tail"]) == tuple(c["tails"]), c["id"]
        tails.add(tuple(c["tails"])); grouped.add(g["grouped"])
    assert tails == {(0, 0), (0, 1), (1, 0), (1, 1)} and 1 in grouped
    assert any(c.get("nt_cols", 0) > c["in"] for c in T.GROUP)


# forms that NO shape selects: reachable through these switches only, run on the device by test_gpu_gemm16.test_env_only_forms
ENV_ONLY = {
    "ORX_GEMM16_TILE": "1 / 3: a configuration at shapes that would take the other; 2: the 128 x 128 tile (LDS-DMA with two stages, or register-staged)",
    "ORX_GEMM16_DMA": "0: the register-staged gemm16_nt_kernel in its three configurations; 2: two LDS-DMA stages",
    "ORX_GEMM16_TN_DMA": "0: the register-staged gemm16_tn_kernel; 2 / 3: the four-wavefront LDS-DMA kernel alone (by default only inside the grouped launch)",
    "ORX_GEMM16_WAVE_TILE": "128: the 256 x 128 tile on four wavefronts",
    "ORX_GEMM16_NTS": "0 / 1: ordinary / nontemporal output stores of the LDS-DMA forms and the grouped launch (default 2: write-through)",
    "ORX_GEMM16_NO_MASK": "no relu masks: orx_gemm16_nt refuses mask arguments",
}


def test_env_only_forms_are_listed_and_selected():
    used = {k for env, _ in T.ENV_SETS.values() for k in env}
    assert used == set(ENV_ONLY)
    forms = set()
    for name, (env, cases) in T.ENV_SETS.items():
        e = {k: v for k, v in os.environ.items() if not k.startswith("ORX_GEMM16_")}
        e.update(env)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gemm16_worker.py"), name, "--plan-only"], env=e, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and f"DONE {len(cases)}" in r.stdout, f"{name}: {r.stdout[-2000:]}\n{r.stderr[-2000:]}"
        for kind, c in cases:
            f = c.get("expect_form", {})
            if kind == "nt":
                forms.add(("nt", f.get("cfg"), f.get("stages"), f.get("wave_tile", 64)))
            elif kind == "tn":
                forms.add(("tn", f["form"]))
    assert {("nt", 2, 2, 64), ("nt", 2, 0, 64), ("nt", 1, 0, 64), ("nt", 3, 0, 64), ("nt", 1, 2, 64), ("nt", 3, 2, 64), ("nt", 1, 3, 128),
            ("tn", 0), ("tn", 2), ("tn", 3)} <= forms
