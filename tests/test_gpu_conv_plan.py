"""The work partition of the 3x3 convolution launches (csrc/conv3x3.hip: whole rounds through the XCD permutation, the span table of
the last round, partial tiles and the fix-up launch; csrc/conv3x3_wgrad.hip: S = grid / blocks pixel ranges) on the device, in EXACT
arithmetic.  Operands are small integers (|x| <= 16, |w| <= 4, |gy| <= 16): one bf16 piece each, every product and every partial sum
an integer below 2^24 (asserted), so the float64 result of torch's operator cast to float32 is THE answer whatever the summation order
and torch.equal is the criterion -- no tolerance; equality across grids follows.  Each case of tests/conv_plan_cases.py runs on its own
grid (ops.set_reserved_cus, restored afterwards), which makes whole rounds, grids that are no multiple of 8 and every kind of span
reachable with a few dozen 7 x 7 or 14 x 14 images; tests/test_conv_plan_host.py asserts that the list contains every regime for every
kernel family, here the plan of the device at that grid is asserted to be the plan those regimes were read from.

Not here: the equal-span fallback on the device.  A launch takes it only under stream capture of a shape it has not seen; its index
logic is replayed on the host (tests/test_conv_plan_host.py, both span modes)."""
import contextlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_plan_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@contextlib.contextmanager
def grid(G):
    """the persistent grids sized for G compute units (0: all of them); the full grid is restored afterwards"""
    from shapeclipper_amd import ops
    torch.cuda.synchronize()
    try:
        full = ops.set_reserved_cus(0)
        if G:
            assert 8 <= G < full and ops.set_reserved_cus(full - G) == G
        yield G or full
    finally:
        torch.cuda.synchronize()
        ops.set_reserved_cus(0)


def ints(shape, bound, seed):
    return C.int_tensor(shape, bound, torch.Generator().manual_seed(seed), DEV)


def same(got, ref64, what):
    ref = ref64.float()
    assert torch.equal(ref.double(), ref64), "the reference is not a float32 tensor: " + what
    assert got.shape == ref.shape and torch.equal(got, ref), "%s: %d of %d elements differ, largest difference %g" % (
        what, int((got != ref).sum()), ref.numel(), float((got - ref).abs().max()))


def wgrad_checks(stride, side, cin, cout, batch, seed, what):
    """conv3x3_backward_weight, plain and split, or conv3x3s2_backward_weight, on integer operands of the given shape"""
    from shapeclipper_amd import ops
    so = side // stride
    C.assert_exact_sum(batch * so * so, C.X_MAX, C.GY_MAX)
    x, gy = ints((batch, cin, side, side), C.X_MAX, seed + 3), ints((batch, cout, so, so), C.GY_MAX, seed + 4)
    dw64 = torch.nn.grad.conv2d_weight(x.double(), (cout, cin, 3, 3), gy.double(), stride, 1)
    if stride == 2:
        same(ops.conv3x3s2_backward_weight(gy, x), dw64, what + " stride-2 weight gradient")
    else:
        same(ops.conv3x3_backward_weight(gy, x), dw64, what + " weight gradient")
        same(ops.conv3x3_backward_weight(gy, x, split=True), dw64, what + " weight gradient (split)")


def run_case(case):
    """every entry point of the case's family on the current grid; returns the forward result (compared across a table release)"""
    from shapeclipper_amd import _lib, ops
    family, side, cin, cout, batch, _ = case
    what = C.case_id(case)
    seed = side + cin + cout + batch
    red = C.reduce_channels(family, cin, cout)
    C.assert_exact_sum((4 if family == "s2bd" else 9) * red, C.X_MAX, C.W_MAX, extra=C.X_MAX)
    w = ints((cout, cin, 3, 3), C.W_MAX, seed)
    both64 = cin % 64 == 0 and cout % 64 == 0
    if family == "s2bd":
        gy = ints((batch, cout, side // 2, side // 2), C.GY_MAX, seed + 1)
        gx = ops.conv3x3s2_backward_data(gy, w, side)
        same(gx, torch.nn.grad.conv2d_input((batch, cin, side, side), w.double(), gy.double(), 2, 1), what + " backward-data")
        return gx
    x = ints((batch, cin, side, side), C.X_MAX, seed + 1)
    if family == "s2fwd":
        y = ops.conv3x3s2_forward(x, w)
        same(y, torch.nn.functional.conv2d(x.double(), w.double(), None, 2, 1), what + " forward")
        if both64:
            wgrad_checks(2, side, cin, cout, batch, seed, what)
        return y
    split = family == "split"
    y64 = torch.nn.functional.conv2d(x.double(), w.double(), None, 1, 1)
    y = ops.conv3x3_forward(x, w, split=split)
    same(y, y64, what + " forward")
    # backward-data with the plan of the case: a filter [cin][cout][3][3], whose flipped image reduces over cin and writes cout channels
    wb, gy = ints((cin, cout, 3, 3), C.W_MAX, seed + 2), ints((batch, cin, side, side), C.GY_MAX, seed + 5)
    same(ops.conv3x3_backward_data(gy, wb, split=split), torch.nn.grad.conv2d_input((batch, cout, side, side), wb.double(), gy.double(), 1, 1),
         what + " backward-data")
    # the addend is applied in both store paths: conv_store_tile (whole tiles) and the fix-up launch (shared tiles)
    lib = _lib.load()
    addend, out = ints(tuple(y.shape), C.X_MAX, seed + 6), torch.full_like(y, float("nan"))
    pack = ops.conv3x3_pack(w, side, False, split)
    _lib.check(lib.sc_conv3x3_forward_add(_lib.ptr(x), _lib.ptr(pack), _lib.ptr(addend), _lib.ptr(out), _lib.ptr(ops._conv_workspace(x.device, side, split)),
                                          batch, cin, cout, side, int(split), _lib.stream()), "sc_conv3x3_forward_add")
    same(out, y64 + addend.double(), what + " forward + addend")
    if both64:
        wgrad_checks(1, side, cin, cout, batch, seed, what)
    return y


@pytest.mark.parametrize("case", C.GPU_CASES, ids=C.case_id)
def test_partition_exact(case):
    family, side, cin, cout, batch, G = case
    with grid(G) as cus:
        p = C.plan(family, side, batch, cin, cout, 0)                        # what the launches on this device follow now
        assert p["G"] == cus and p == C.plan(family, side, batch, cin, cout, cus), "the device's plan is not the plan of a grid of %d" % cus
        print("%s: tiles %d, K-steps %d, rounds %d, tail tiles %d on %d workgroups: %s" % (
            C.case_id(case), p["tiles"], p["nk"], p["rounds"], p["tail_tiles"], p["G"], " ".join(sorted(C.regimes(family, side, batch, cin, cout, p)))))
        run_case(case)


@pytest.mark.parametrize("case", C.WGRAD_CASES, ids=C.wgrad_id)
def test_weight_gradient_ranges_exact(case):
    """S = max(1, grid / blocks) pixel ranges per 64 x 64 block of the weight gradient, on shrunk grids"""
    stride, side, cin, cout, batch, G = case
    with grid(G):
        wgrad_checks(stride, side, cin, cout, batch, sum(case), C.wgrad_id(case))


def test_release_tables_then_same_values():
    """sc_conv3x3_release_tables frees the span tables of every shape this module has launched; the next launch rebuilds its table and
    computes the same values."""
    from shapeclipper_amd import _lib
    case = C.GPU_CASES[0]
    assert C.plan(case[0], case[1], case[4], case[2], case[3], case[5])["table"] == 1
    with grid(case[5]):
        before = run_case(case).clone()
        torch.cuda.synchronize()
        assert _lib.load().sc_conv3x3_release_tables() == 0
        assert torch.equal(run_case(case), before)
        torch.cuda.synchronize()
        assert _lib.load().sc_conv3x3_release_tables() == 0                  # twice in a row, nothing in between
        assert _lib.load().sc_conv3x3_release_tables() == 0
        assert torch.equal(run_case(case), before)
