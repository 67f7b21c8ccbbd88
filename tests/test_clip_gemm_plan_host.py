"""The CLIP GEMM launch rule (gemm_plan in csrc/clip_vit.hip, exported as sc_gemm_plan) on the host: no GPU.  The rule picks between seven
kernels and three tail hand-overs from M, N, K, the epilogue and the CU count; the CU count is passed (256, the MI355X) so nothing here
asks a device.  Checked: an expected plan per branch, the plans of the product's own GEMMs, invariants over a sweep against a Python
restatement of the rule, the refusals, and -- in a child process, because the SC_GEMM_* overrides are read once -- the one override that
makes gemm256_kernel reachable."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

assert not [k for k in os.environ if k.startswith("SC_GEMM_")], "the SC_GEMM_* overrides are read once per process: unset them for this module"

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CUS = 256
MAIN = ("t64", "t128", "persist", "gemm8p", "gemm8p_192", "gemm256")
TAIL = (None, "thin", "t64")
INVALID = 1                       # hipErrorInvalidValue


def plan(epi, M, N, K, cus=CUS):
    """(main kernel, its rows, tail kernel, its rows, the main kernel's tiles) or the refusal's status"""
    from shapeclipper_amd import _lib
    out = (ctypes.c_int * 5)(*([-1] * 5))
    rc = _lib.load().sc_gemm_plan(epi, M, N, K, cus, out)
    if rc:
        assert list(out) == [-1] * 5, "a refusal wrote a plan"
        return rc
    return MAIN[out[0]], out[1], TAIL[out[2]], out[3], out[4]


def rule(epi, M, N, K, cus=CUS):
    """The rule restated with its default thresholds (include/shapeclipper_hip.h)."""
    cdiv = lambda a, b: (a + b - 1) // b
    t128, t256, t192 = cdiv(N, 128) * cdiv(M, 128), (N // 256) * cdiv(M, 256), (N // 192) * cdiv(M, 256)
    fits = (M + 256) * N * 4 < 2 ** 32 and (M + 256) * K * 2 < 2 ** 32 and N * K * 2 < 2 ** 32
    if N % 256 == 0 and M >= 2048 and t256 >= 200 and fits:
        rem8, t_main, grid = M % 256, (M // 256) * (N // 256), cus // 8 * 8
        if 0 < rem8 <= 64 and t_main > 0 and grid > 0 and N % 32 == 0 and K % 256 == 0 and cdiv(t256, grid) > cdiv(t_main, grid):
            return "gemm8p", M - rem8, "thin", rem8, t_main
        return "gemm8p", M, None, 0, t256
    if epi in (0, 1) and N % 192 == 0 and M >= 2048 and 180 <= t192 <= 256 and fits:
        return "gemm8p_192", M, None, 0, t192
    if N % 256 == 0 and M >= 2048 and t256 >= 128 and t256 * 100 >= cdiv(t256, 256) * 256 * 85:
        return "gemm256", M, None, 0, t256
    if t128 < 384:
        return "t64", M, None, 0, cdiv(N, 64) * cdiv(M, 64)
    if N % 8:
        return "t128", M, None, 0, t128
    rem, ntn, t_full = M % 128, cdiv(N, 128), cdiv(N, 128) * (M // 128)
    if rem and t_full > 0 and N % 32 == 0 and K % 256 == 0 and cdiv(t128, 512) > cdiv(t_full, 512):
        return "persist", M - rem, "thin", rem, t_full
    main_mt = t128 // 512 * 512 // ntn
    if rem == 0 and t128 > 512 and 0 < t128 % 512 and (t128 % 512) * 100 < 512 * 25 and main_mt > 0:
        return "persist", main_mt * 128, "t64", M - main_mt * 128, main_mt * ntn
    return "persist", M, None, 0, t128


ALL = (0, 1, 2, 3)
# (M, N, K), epilogues, main, main rows (None: M), tail, tail rows, tiles (None: not stated).  One row per branch.
TABLE = [((M, N, K), ALL, "t64", None, None, 0, None) for M, N, K in [(1, 64, 64), (33, 200, 128), (70, 100, 192), (130, 71, 256), (41, 512, 768)]] + [
    ((5377, 1027, 64), ALL, "t128", None, None, 0, 387),
    ((6144, 1024, 64), ALL, "persist", None, None, 0, 384),
    ((7297, 1032, 192), ALL, "persist", None, None, 0, 522),
    ((10368, 1024, 192), ALL, "persist", None, None, 0, 648),
    ((8193, 1024, 256), ALL, "persist", 8192, "thin", 1, None),
    ((8319, 1024, 768), ALL, "persist", 8192, "thin", 127, None),
    ((8320, 1024, 64), ALL, "persist", 8192, "t64", 128, None),
    ((7296, 1032, 192), ALL, "persist", 7168, "t64", 128, 504),
    ((9216, 960, 128), (2, 3), "persist", 8192, "t64", 1024, None),
    ((9216, 960, 128), (0, 1), "gemm8p_192", None, None, 0, None),
    ((2049, 6400, 128), ALL, "gemm8p", None, None, 0, None),
    ((8257, 2048, 192), ALL, "gemm8p", None, None, 0, 264),
    ((8193, 2048, 256), ALL, "gemm8p", 8192, "thin", 1, None),
    ((8256, 2048, 256), ALL, "gemm8p", 8192, "thin", 64, None),
    ((8257, 2048, 256), ALL, "gemm8p", None, None, 0, None),             # a rem8 of 65 is not peeled
    ((11265, 768, 64), (0, 1), "gemm8p_192", None, None, 0, None),
    ((11265, 768, 64), (2, 3), "persist", None, None, 0, 534),
]


@pytest.mark.parametrize("shape,epis,main,main_rows,tail,tail_rows,tiles", TABLE, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) and len(v) == 3 else None)
def test_one_plan_per_branch(shape, epis, main, main_rows, tail, tail_rows, tiles):
    M, N, K = shape
    for epi in epis:
        got = plan(epi, M, N, K)
        assert got[:4] == (main, M if main_rows is None else main_rows, tail, tail_rows), (shape, epi, got)
        assert tiles is None or got[4] == tiles, (shape, epi, got)
        assert got == rule(epi, M, N, K), (shape, epi, got)


def tower_gemms(B, T, D, mlp, Kp, proj):
    M = B * T
    return {"patch": (0, B * (T - 1), D, Kp), "qkv": (3, M, 3 * D, D), "out_proj": (1, M, D, D), "fc1": (2, M, mlp, D), "fc2": (1, M, D, mlp),
            "proj": (0, B, proj, D)}


VIT_B32 = dict(T=50, D=768, mlp=3072, Kp=3072, proj=512)
VIT_L14 = dict(T=257, D=1024, mlp=4096, Kp=640, proj=768)          # 3 * 14 * 14 = 588 patch values, padded to the K granularity
PRODUCT = [
    (VIT_B32, (1, 8, 32), ("t64",) * 5),
    (VIT_B32, (256,), ("gemm8p_192", "gemm8p", "gemm8p_192", "gemm8p", "gemm8p_192")),
    (VIT_L14, (1,), ("t64",) * 5),
    (VIT_L14, (8,), ("t64", "persist", "t64", "persist+thin", "t64")),
    (VIT_L14, (32,), ("persist", "gemm8p", "persist+thin", "gemm8p+thin", "persist+thin")),
    (VIT_L14, (256,), ("gemm8p",) * 5),
]


@pytest.mark.parametrize("model,batches,want", PRODUCT, ids=["B32-small", "B32-256", "L14-1", "L14-8", "L14-32", "L14-256"])
def test_plans_of_the_towers_own_gemms(model, batches, want):
    for B in batches:
        g = tower_gemms(B, **model)
        got = {k: plan(*v) for k, v in g.items()}
        names = tuple(got[k][0] + ("+" + got[k][2] if got[k][2] else "") for k in ("patch", "qkv", "out_proj", "fc1", "fc2"))
        assert names == want, (B, got)
        assert got["proj"][0] == "t64" and got["proj"][2] is None, (B, got["proj"])
        for k, v in g.items():
            assert got[k][1] + got[k][3] == v[1]


SWEEP_M = sorted(set(range(1, 13001, 61)) | {m for c in range(128, 13001, 128) for m in (c - 1, c, c + 1)})
SWEEP_N = (64, 71, 100, 192, 200, 256, 384, 512, 520, 768, 960, 1024, 1027, 1032, 1536, 2048, 2304, 3072, 3100, 4096, 6144, 6400)
SWEEP_K = (64, 192, 256, 768)


def test_invariants_over_a_sweep():
    seen = set()
    for N in SWEEP_N:
        for K in SWEEP_K:
            for epi in ALL:
                for M in SWEEP_M:
                    main, m0, tail, m1, tiles = got = plan(epi, M, N, K)
                    what = (epi, M, N, K, got)
                    assert got == rule(epi, M, N, K), what
                    assert m0 > 0 and m1 >= 0 and m0 + m1 == M and tiles > 0 and (m1 > 0) == (tail is not None), what
                    if tail == "thin":
                        assert main in ("persist", "gemm8p") and N % 32 == 0 and K % 256 == 0 and m1 <= (64 if main == "gemm8p" else 127), what
                    if tail == "t64":
                        assert main == "persist" and M % 128 == 0 and m0 % 128 == 0, what
                    if main == "gemm8p":
                        assert N % 256 == 0, what
                    if main == "gemm8p_192":
                        assert N % 192 == 0 and epi in (0, 1), what
                    if main == "persist":
                        assert N % 8 == 0, what
                    assert main != "gemm256", what       # with the default thresholds every gemm256 shape goes to gemm8p first
                    seen.add((main, tail))
    assert seen == {("t64", None), ("t128", None), ("persist", None), ("persist", "thin"), ("persist", "t64"), ("gemm8p", None),
                    ("gemm8p", "thin"), ("gemm8p_192", None)}, seen


def test_cu_count_moves_only_the_gemm8p_tail():
    """8224 x 4096 (fc1 of ViT-L/14 at batch 32): 33 x 16 tiles open a third round of 256 workgroups, not of 304."""
    assert plan(2, 8224, 4096, 1024, 256) == ("gemm8p", 8192, "thin", 32, 512)
    assert plan(2, 8224, 4096, 1024, 304) == ("gemm8p", 8224, None, 0, 528)
    assert plan(2, 8224, 4096, 1024, 7) == ("gemm8p", 8224, None, 0, 528)          # fewer than 8 CUs: no round to count
    for cus in (8, 64, 304):
        assert plan(1, 8224, 1024, 1024, cus) == plan(1, 8224, 1024, 1024, 256) == ("persist", 8192, "thin", 32, 512)


def test_refusals():
    for epi, M, N, K in [(0, 0, 64, 64), (0, -1, 64, 64), (0, 64, 0, 64), (0, 64, -64, 64), (0, 64, 64, 0), (0, 64, 64, -64), (0, 64, 64, 32),
                         (0, 64, 64, 100), (3, 8192, 2048, 65), (-1, 64, 64, 64), (4, 64, 64, 64), (7, 64, 64, 64), (7, 12800, 3072, 768)]:
        assert plan(epi, M, N, K) == INVALID, (epi, M, N, K)
    from shapeclipper_amd import _lib
    assert _lib.load().sc_gemm_plan(0, 64, 64, 64, CUS, None) == INVALID
    assert "sc_gemm_plan" in _lib.TIMING_SKIP


CHILD = """
import ctypes, json, sys
sys.path.insert(0, %r)
from shapeclipper_amd import _lib
lib, out = _lib.load(), (ctypes.c_int * 5)()
res = []
for epi, M, N, K in json.loads(sys.argv[1]):
    rc = lib.sc_gemm_plan(epi, M, N, K, 256, out)
    res.append([rc] + list(out))
print(json.dumps(res))
"""


def test_raised_g8_min_reaches_gemm256_and_turns_the_192_form_off():
    cases = [(e, 7168, 2048, 64) for e in ALL] + [(e, 7100, 2048, 192) for e in ALL] + [(0, 11265, 768, 64)]
    env = dict(os.environ, SC_GEMM_G8_MIN="10000000000000")
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT, json.dumps(cases)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for (epi, M, N, K), g in zip(cases[:8], got[:8]):
        assert g == [0, MAIN.index("gemm256"), M, 0, 0, 8 * ((M + 255) // 256)], (epi, M, N, K, g)
    assert got[8] == [0, MAIN.index("persist"), 11265, 0, 0, 534], got[8]
