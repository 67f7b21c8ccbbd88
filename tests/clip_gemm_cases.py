"""The harness tests/test_gpu_clip_gemm.py runs every CLIP GEMM case through (sc_gemm_bf16 / sc_gemm_f16), and -- run as a program -- the
child process that puts gemm256_kernel through the same checks with SC_GEMM_G8_MIN raised (the SC_GEMM_* overrides are read once per
process, so the parent cannot reach that kernel itself).

Every call:
  * `out` lives inside one buffer between two canaries of 4096 elements; it starts as NaN (epilogues 0, 2, 3) or as the residual (1).
    After the call both canaries are intact and no NaN is left, so every row range of a split plan was written (epilogue 1: the rows
    of the main and of the tail kernel both differ from the residual).
  * A and W are the leading rows of buffers whose last GUARD rows are NaN (same allocation: nothing is read out of bounds).  The kernels
    clamp rows past M and N to the last valid row; one that reads a guard row instead and uses it leaves a NaN in `out`.
Operands are normal 16-bit numbers: what the MFMA does with 16-bit subnormal operands is the hardware's and not under test."""
import json
import os
import sys

import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))

DEV = "cuda:0"
CANARY, GUARD = 4096, 256
ALL = (0, 1, 2, 3)
TD = {"fp16": torch.float16, "bf16": torch.bfloat16}
U = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}                  # half an ulp of a normal 16-bit value, relative
FLOOR = {"fp16": 2.0 ** -25, "bf16": 0.0}                    # half the smallest fp16 subnormal
TINY = {"fp16": 2.0 ** -14, "bf16": 2.0 ** -126}             # smallest normal
MAIN = ("t64", "t128", "persist", "gemm8p", "gemm8p_192", "gemm256")
TAIL = (None, "thin", "t64")
GELU_DEV = {}                                                # largest measured fp32 deviation of QuickGELU per dtype (printed)


def plan(epi, M, N, K, cus=0):
    """(main kernel, its rows, tail kernel, its rows, tiles) as sc_gemm_plan reports it; cus = 0: the device's count"""
    import ctypes
    from shapeclipper_amd import _lib
    out = (ctypes.c_int * 5)()
    rc = _lib.load().sc_gemm_plan(epi, M, N, K, cus, out)
    assert rc == 0, (rc, epi, M, N, K)
    return MAIN[out[0]], out[1], TAIL[out[2]], out[3], out[4]


def assert_plan(epis, M, N, K, main, main_rows=None, tail=None, tail_rows=0):
    for epi in epis:
        got = plan(epi, M, N, K)
        assert got[:4] == (main, M if main_rows is None else main_rows, tail, tail_rows), \
            "(%d, %d, %d) epi %d was built for %s + %s, this device plans %r" % (M, N, K, epi, main, tail, got)
    return got


def guarded(x):
    """x [rows][K] -> the same rows at the head of a buffer that ends in GUARD rows of NaN"""
    buf = torch.full((x.shape[0] + GUARD, x.shape[1]), float("nan"), dtype=x.dtype, device=x.device)
    buf[:x.shape[0]] = x
    return buf[:x.shape[0]]


def run(dtype, epi, A, W, bias, resid):
    """One GEMM call in the harness of the module docstring; returns out [M][N] (fp32 for epilogues 0 / 1, 16 bit for 2 / 3)."""
    from shapeclipper_amd import _lib
    lib = _lib.load()
    (M, K), N = A.shape, W.shape[0]
    assert W.shape[1] == K and A.dtype == W.dtype == TD[dtype] and A.is_contiguous() and W.is_contiguous()
    odt = torch.float32 if epi in (0, 1) else TD[dtype]
    buf = torch.full((M * N + 2 * CANARY,), 7.0, dtype=odt, device=DEV)
    out = buf[CANARY:CANARY + M * N].view(M, N)
    if epi == 1:
        out.copy_(resid)
    else:
        out.fill_(float("nan"))
    fn = lib.sc_gemm_f16 if dtype == "fp16" else lib.sc_gemm_bf16
    rc = fn(epi, _lib.ptr(A), _lib.ptr(W), _lib.ptr(bias), _lib.ptr(out), M, N, K, _lib.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    what = (dtype, epi, M, N, K, "bias" if bias is not None else "no bias")
    assert (buf[:CANARY] == 7.0).all(), ("written in front of out", what)
    assert (buf[CANARY + M * N:] == 7.0).all(), ("written behind out", what)
    nan = torch.isnan(out)
    if nan.any():
        rows = nan.any(1).nonzero().flatten()
        raise AssertionError(("NaN left in out: %d elements, rows %d..%d (not written, or a guard row was used)"
                              % (int(nan.sum()), int(rows[0]), int(rows[-1])), what))
    return out


def assert_ranges_written(out, resid, K, what):
    """epilogue 1 starts from the residual, not from NaN: the rows of the main kernel and the rows of the tail kernel must both have moved"""
    M, N = out.shape
    _, m0, tail, m1, _ = plan(1, M, N, K)
    for name, lo, hi in (("main", 0, m0), (tail, m0, m0 + m1)):
        assert hi == lo or bool((out[lo:hi] != resid[lo:hi]).any()), ("rows %d..%d (%s kernel) still hold the residual" % (lo, hi - 1, name), what)


def bits(x):
    return x.contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int16)


def assert_bits(out, want, what, hint=None):
    bad = bits(out) != bits(want)
    if bad.any():
        r, c = (int(v) for v in bad.nonzero()[0])
        msg = "%d of %d elements differ; first at row %d col %d: got %r, want %r" % (
            int(bad.sum()), bad.numel(), r, c, float(out[r, c]), float(want[r, c]))
        raise AssertionError((msg, what) if hint is None else (msg, hint(bad), what))


def gelu_term(v64):
    """Largest relative deviation of a torch fp32 evaluation of v / (1 + exp(-1.702 v)) from float64 over these v (CPU: this is the
    reference, not the kernel)."""
    v = v64.cpu()
    f64 = v / (1.0 + torch.exp(-1.702 * v))
    v32 = v.float()
    f32 = v32 / (1.0 + torch.exp(-1.702 * v32))
    return float(((f32.double() - f64).abs() / f64.abs()).nan_to_num(0.0).max())


def assert_bound(out, want, ref, dtype, epi, what):
    """epilogues 0 / 1: the project's own bar, 1e-5 of max |ref|.  3: one correct rounding of a value that carries that fp32 error,
    U |want| + 1e-5 max |ref| (+ half the smallest subnormal in fp16).  2: that, plus four times the measured fp32 deviation of the
    QuickGELU formula over this case's own values (four times, because __expf is not torch's exp).  Measured over the cases of
    tests/test_gpu_clip_gemm.py: 5.1e-07 .. 4.04e-06 per case."""
    scale = float(ref.abs().max())
    tol = torch.full_like(want, 1e-5 * scale)
    if epi in (2, 3):
        tol += U[dtype] * want.abs() + FLOOR[dtype]
    if epi == 2:
        dev = gelu_term(ref)
        GELU_DEV[dtype] = max(GELU_DEV.get(dtype, 0.0), dev)
        tol += 4.0 * dev * want.abs()
    err = (out.double() - want).abs()
    worst = float((err / tol).max())
    print("GEMM %s: max |err| %.3e, worst err / bound %.3f%s" % (what, float(err.max()), worst, ", fp32 QuickGELU deviation %.2e" % dev if epi == 2 else ""))
    assert worst <= 1.0, (worst, float(err.max()), scale, what)


def quick_gelu64(v):
    return v / (1.0 + torch.exp(-1.702 * v))


def check_integer(M, N, K, dtype, epis=ALL):
    """Integer operands in [-4, 4], bias and residual in [-64, 64]: exact in both 16-bit formats, and with K <= 768 every partial sum is
    below 16 * 768 + 128 < 2^24, so the fp32 result is exact in ANY summation order.  Epilogues 0 / 1 equal the integer matmul (taken in
    float64, where it is exact too) bit for bit, 3 its one rounding to 16 bits.  Epilogue 2 is not exact on any operands: its harness
    checks (canaries, every element written) run here, its values are check_random's.  With and without bias."""
    assert K <= 768
    g = torch.Generator(device=DEV).manual_seed(1000 * M + N + K)
    td = TD[dtype]
    A = guarded(torch.randint(-4, 5, (M, K), generator=g, device=DEV).to(td))
    W = guarded(torch.randint(-4, 5, (N, K), generator=g, device=DEV).to(td))
    bias = torch.randint(-64, 65, (N,), generator=g, device=DEV).float()
    resid = torch.randint(-64, 65, (M, N), generator=g, device=DEV).float()
    base = A.double() @ W.double().t()
    assert float(base.abs().max()) + 128 < 2 ** 24
    for b in (bias, None):
        ref = base + bias.double() if b is not None else base
        for epi in epis:
            what = (dtype, "integers", epi, M, N, K, "bias" if b is not None else "no bias")
            out = run(dtype, epi, A, W, b, resid)
            if epi == 0:
                assert_bits(out, ref.float(), what)
            elif epi == 1:
                assert_ranges_written(out, resid, K, what)
                assert_bits(out, (ref + resid.double()).float(), what)
            elif epi == 3:
                assert_bits(out, ref.float().to(td), what)


def check_one_hot(M, N, K, dtype, epis=(0, 3)):
    """A[m, :] is 1 at k(m) = (7 m + 3) % K and 0 elsewhere, W[n, k] = ((31 n + 17 k) % 9) - 4: out[m, n] must be exactly W[n, k(m)], and a
    failure names the K-chunks (8 values: one LDS-DMA / swizzle slot) and K-steps (64) of the rows that are wrong."""
    td = TD[dtype]
    m, n, k = torch.arange(M, device=DEV), torch.arange(N, device=DEV), torch.arange(K, device=DEV)
    km = (7 * m + 3) % K
    A = torch.zeros(M, K, device=DEV, dtype=td)
    A[m, km] = 1.0
    Wv = ((n[:, None] * 31 + k[None, :] * 17) % 9 - 4).to(td)
    A, W = guarded(A), guarded(Wv)
    want = Wv.float()[:, km].t().contiguous()

    def hint(bad):
        ks = km[bad.any(1)]
        return "rows wrong: %d; their K-steps %s, K-chunks within the step %s" % (
            int(bad.any(1).sum()), sorted(set((ks // 64).tolist()))[:12], sorted(set((ks % 64 // 8).tolist())))

    for epi in epis:
        out = run(dtype, epi, A, W, None, None)
        assert_bits(out, want if epi == 0 else want.to(td), (dtype, "one-hot", epi, M, N, K), hint)


def check_random(M, N, K, dtype, epis=ALL):
    """Random operands at the scales of test_gemm_256_tiles_all_epilogues against float64 (assert_bound), each call made twice: the
    summation order is fixed by design, so two outputs that differ in a bit are a race in the hand-counted pipeline."""
    g = torch.Generator(device=DEV).manual_seed(M + N)
    td = TD[dtype]

    def normal16(x):                                        # no 16-bit subnormal operands (module docstring)
        x = x.to(td)
        small = x.abs() < TINY[dtype]
        return guarded(torch.where(small, torch.full_like(x, TINY[dtype]), x))

    A = normal16(torch.randn(M, K, generator=g, device=DEV) * 0.5)
    W = normal16((torch.randn(N, K, generator=g, device=DEV) + torch.arange(N, device=DEV)[:, None] * 0.002) * 0.1)
    bias = torch.randn(N, generator=g, device=DEV)
    resid = torch.randn(M, N, generator=g, device=DEV)
    base = A.double() @ W.double().t()
    for b in (bias, None):
        ref = base + bias.double() if b is not None else base
        for epi in epis:
            what = (dtype, "random", epi, M, N, K, "bias" if b is not None else "no bias")
            out = run(dtype, epi, A, W, b, resid)
            again = run(dtype, epi, A, W, b, resid)
            assert torch.equal(bits(out), bits(again)), ("two calls differ in %d elements" % int((bits(out) != bits(again)).sum()), what)
            if epi == 1:
                assert_ranges_written(out, resid, K, what)
            want = ref + resid.double() if epi == 1 else quick_gelu64(ref) if epi == 2 else ref
            assert_bound(out, want, ref, dtype, epi, what)


GEMM256_SHAPES = ((7168, 2048, 64), (7100, 2048, 192))


def main():
    """The gemm256 child: SC_GEMM_G8_MIN is raised in its environment.  Prints the plans as one JSON line, then every failed check; exit
    status 0: all passed, 1: a check failed, 2: anything else (nothing more is started on the GPU after that)."""
    plans = [[list(plan(epi, *s)) for epi in ALL] for s in GEMM256_SHAPES]
    print("PLANS " + json.dumps(plans), flush=True)
    if any(p[0] != "gemm256" for ps in plans for p in ps):
        return 1
    failed = 0
    for s in GEMM256_SHAPES:
        for dtype in ("fp16", "bf16"):
            for check in (check_integer, check_random):
                try:
                    check(*s, dtype)
                except AssertionError as e:
                    failed += 1
                    print("FAILED %s %r %s: %r" % (check.__name__, s, dtype, e), flush=True)
                except Exception as e:
                    print("ERROR %s %r %s: %r" % (check.__name__, s, dtype, e), flush=True)
                    return 2
    print("QuickGELU fp32 deviation %r" % GELU_DEV)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
