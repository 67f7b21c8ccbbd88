"""Every branch of the CLIP GEMM launch rule (gemm_plan in csrc/clip_vit.hip) on the device, through the entry points the tower's GEMMs
share (sc_gemm_bf16 / sc_gemm_f16), both 16-bit formats, every epilogue, with and without bias.  Each case first asks sc_gemm_plan for
the plan of its shape ON THIS DEVICE and asserts the branch it was built for, so a case can never silently test another kernel
(tests/test_clip_gemm_plan_host.py holds the same table for 256 CUs without a GPU).  The harness -- canaries on both sides of `out`, NaN
prefill, NaN guard rows behind A and W -- is tests/clip_gemm_cases.py; so are the three checks:

  a. integer operands: bit-exact whatever the summation order (and a one-hot A that names the misplaced K-chunk);
  b. random operands against float64 at derived bounds, each call twice and bit-equal;
  c. gemm256_kernel, which the default thresholds never select, in one child process with SC_GEMM_G8_MIN raised
     (tests/test_gpu_clip_anno.py: tests that start processes run in the suite's last group);
  d. sc_f32_to_bf16 / sc_f32_to_f16 against torch's CPU conversion, bit-exact except for NaN payloads.

What each row reaches that nothing reached before:
  (33, 200, 128), (70, 100, 192), (130, 71, 256)   the element-wise epilogue of gemm_bf16_kernel<64> (partial N tile; N % 8 != 0)
  (5377, 1027, 64)        gemm_bf16_kernel<128>, its element-wise epilogue with 2-byte stores at an odd row pitch
  (7297, 1032, 192)       persistent kernel: 522 tiles on 512 workgroups -- a second tile, the next-tile prefetch, the stage parity across
                          tiles of three K-steps -- and its partial last N tile (1032 = 8 x 128 + 8)
  (10368, 1024, 192), (11265, 768, 64)   second tiles with an odd / a single K-step, ragged last row tile
  (8193 / 8319, 1024, .)  gemm_thin_kernel at 1 and 127 rows, K = 256: one 16-wide K-step per wave
  (8320, 1024, 64), (7296, 1032, 192), (9216, 960, 128)   the 64-wide tail behind the persistent kernel, fp32 epilogues included
  (8257, 2048, 192)       gemm8p: 264 tiles on 256 workgroups, three K-tiles per output tile
  (8193 / 8256, 2048, 256)   gemm_thin_kernel behind gemm8p at 1 and 64 rows

Operands are normal 16-bit numbers: the MFMA's treatment of 16-bit subnormal operands is the hardware's and out of scope, as is any
operand alignment other than what torch's allocations give.

Measured (printed by every case): a torch fp32 evaluation of QuickGELU deviates from float64 by at most 4.04e-06 relative over these cases'
own values (bf16; fp16: 3.95e-06; per case 5.1e-07 .. 4.04e-06: for v << 0 the formula amplifies the fp32 rounding of v by 1 + 1.702 |v|);
the bound allows four times that next to the 16-bit rounding of 4.9e-04 / 3.9e-03.  The worst error of any case is 0.992 of its bound
(epilogue 3: a correct rounding is up to half an ulp off).  The 125 cases of the module run in 16-21 s on the MI355X (two runs), none longer than 1.0 s (the
gemm256 child: 5.2 s, most of it the child's start)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_gemm_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

ALL = C.ALL
DTYPES = ["fp16", "bf16"]
# (M, N, K), epilogues, main kernel, its rows (None: M), tail kernel, its rows
ROWS = [((M, N, K), ALL, "t64", None, None, 0) for M, N, K in [(1, 64, 64), (33, 200, 128), (70, 100, 192), (130, 71, 256), (41, 512, 768)]] + [
    ((5377, 1027, 64), ALL, "t128", None, None, 0),
    ((6144, 1024, 64), ALL, "persist", None, None, 0),
    ((7297, 1032, 192), ALL, "persist", None, None, 0),
    ((10368, 1024, 192), ALL, "persist", None, None, 0),
    ((8193, 1024, 256), ALL, "persist", 8192, "thin", 1),
    ((8319, 1024, 768), ALL, "persist", 8192, "thin", 127),
    ((8320, 1024, 64), ALL, "persist", 8192, "t64", 128),
    ((7296, 1032, 192), ALL, "persist", 7168, "t64", 128),
    ((9216, 960, 128), (2, 3), "persist", 8192, "t64", 1024),
    ((9216, 960, 128), (0, 1), "gemm8p_192", None, None, 0),
    ((2049, 6400, 128), ALL, "gemm8p", None, None, 0),
    ((8257, 2048, 192), ALL, "gemm8p", None, None, 0),
    ((8193, 2048, 256), ALL, "gemm8p", 8192, "thin", 1),
    ((8256, 2048, 256), ALL, "gemm8p", 8192, "thin", 64),
    ((8257, 2048, 256), ALL, "gemm8p", None, None, 0),
    ((11265, 768, 64), (0, 1), "gemm8p_192", None, None, 0),
    ((11265, 768, 64), (2, 3), "persist", None, None, 0),
]
IDS = ["%dx%dx%d-epi%s-%s%s" % (*r[0], "".join(map(str, r[1])), r[2], "+" + r[4] if r[4] else "") for r in ROWS]
ONE_HOT = [r for r in ROWS if r[2] in ("t64", "t128", "persist") or r[4] == "thin"]
ONE_HOT_IDS = [i for i, r in zip(IDS, ROWS) if r in ONE_HOT]


def _planned(row):
    (M, N, K), epis, main, main_rows, tail, tail_rows = row
    C.assert_plan(epis, M, N, K, main, main_rows, tail, tail_rows)
    return M, N, K, epis


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_integer_operands_bit_exact(row, dtype):
    M, N, K, epis = _planned(row)
    C.check_integer(M, N, K, dtype, epis)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("row", ONE_HOT, ids=ONE_HOT_IDS)
def test_one_hot_rows_select_one_weight_column(row, dtype):
    M, N, K, epis = _planned(row)
    C.check_one_hot(M, N, K, dtype, [e for e in (0, 3) if e in epis])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_random_operands_vs_float64_twice(row, dtype):
    M, N, K, epis = _planned(row)
    C.check_random(M, N, K, dtype, epis)
    print("largest fp32 QuickGELU deviation so far: %r" % C.GELU_DEV)


def test_refusals_launch_nothing():
    """M, N, K <= 0, K % 64 != 0 and an epilogue outside 0..3 are refused on every branch: `out` keeps its NaN."""
    from shapeclipper_amd import _lib
    lib = _lib.load()
    A = torch.ones(12800, 768, device=C.DEV, dtype=torch.float16)
    W = torch.ones(3072, 768, device=C.DEV, dtype=torch.float16)
    out = torch.full((12800 * 3072,), float("nan"), device=C.DEV)
    for epi, M, N, K in [(0, 0, 64, 64), (0, 64, 0, 64), (0, 64, 64, 0), (0, -64, 64, 64), (0, 64, 64, 32), (7, 64, 64, 64), (-1, 64, 64, 64),
                         (7, 6144, 1024, 64), (7, 12800, 3072, 768), (4, 12800, 768, 768)]:
        for fn in (lib.sc_gemm_bf16, lib.sc_gemm_f16):
            assert fn(epi, _lib.ptr(A), _lib.ptr(W), None, _lib.ptr(out), M, N, K, _lib.stream()) == 1, (epi, M, N, K)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---- d. the fp32 -> 16 bit conversions of the weight preparation ------------------------------------------------------------------------
def _conversion_inputs(dtype):
    """fp32 bit patterns: +-0, +-inf, NaN, ties that round down (even mantissa below) and up (odd), fp32 subnormals, the 16-bit format's
    subnormal range, and each format's overflow edge."""
    pats = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001,
            0x00000001, 0x807FFFFF, 0x00400000, 0x007FFFFF, 0x00800000]              # fp32 subnormals and the smallest normal
    if dtype == "bf16":
        pats += [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF,          # ties at 1 + 2^-8 (down), 1 + 3 * 2^-8 (up)
                 0x00008000, 0x00018000, 0x00010000, 0x007F8000, 0x807F8000,                      # bf16 subnormal range, ties in it
                 0x7F7F0000, 0x7F7F8000, 0x7F7F7FFF, 0x7F7FFFFF, 0xFF7F8000, 0xFF7FFFFF]          # largest finite, the tie above it, FLT_MAX
        vals = []
    else:
        pats += [0x3F801000, 0x3F803000, 0xBF801000, 0xBF803000, 0x3F801001, 0x3F800FFF]          # ties at 1 + 2^-11 (down), 1 + 3 * 2^-11 (up)
        vals = [65504.0, 65519.99, 65520.0, -65520.0, 65536.0, 1e6, -1e6,                         # 65520: the tie that becomes inf
                2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0000001, 3 * 2.0 ** -25, 2.0 ** -26,
                -2.0 ** -24, -2.0 ** -25, 1023.5 * 2.0 ** -24, 1022.5 * 2.0 ** -24, 1e-5, 3.3e-7]  # fp16's subnormal range, ties in it
    x = torch.from_numpy(np.array(pats, dtype=np.uint32).view(np.float32))
    return torch.cat([x, torch.tensor(vals, dtype=torch.float32)])


@pytest.mark.parametrize("dtype", DTYPES)
def test_f32_to_16bit_conversions_match_torch(dtype):
    """n = 1, 255, 256, 257 (one block, its edge) and 4096 * 256 + 257 (more than one sweep of the kernel's grid of at most 4096 blocks),
    a canary behind y.  Random values over the whole exponent range of the 16-bit format, its subnormals included, fill the rest."""
    from shapeclipper_amd import _lib
    lib = _lib.load()
    fn, td = (lib.sc_f32_to_f16, torch.float16) if dtype == "fp16" else (lib.sc_f32_to_bf16, torch.bfloat16)
    special = _conversion_inputs(dtype)
    g = torch.Generator().manual_seed(5)
    big = 4096 * 256 + 257
    lo, hi = (-27.0, 17.0) if dtype == "fp16" else (-135.0, 128.0)
    fill = (torch.randn(big, generator=g) * torch.exp2(torch.rand(big, generator=g, dtype=torch.float64) * (hi - lo) + lo).float())
    for n in (1, 255, 256, 257, big):
        x = fill[:n].clone()
        k = min(n, special.numel())
        x[n - k:] = special[:k]                                # the special values end the array: the last block, the last sweep
        if n == 1:
            x[0] = 65520.0                                     # fp16: the tie that becomes inf; bf16: exact
        want = x.to(td)
        buf = torch.full((n + C.CANARY,), 7.0, dtype=td, device=C.DEV)
        xd = x.to(C.DEV)
        assert fn(_lib.ptr(xd), _lib.ptr(buf), n, _lib.stream()) == 0
        torch.cuda.synchronize()
        assert (buf[n:] == 7.0).all(), (dtype, n, "written behind y")
        got = buf[:n].cpu()
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan), (dtype, n)
        bad = (C.bits(got) != C.bits(want)) & ~nan
        assert not bad.any(), (dtype, n, int(bad.sum()), [(float(x[i]), hex(int(C.bits(got)[i]) & 0xFFFF), hex(int(C.bits(want)[i]) & 0xFFFF))
                                                          for i in bad.nonzero().flatten()[:8].tolist()])
    assert fn(None, None, 0, _lib.stream()) == 0               # n <= 0: nothing to do
