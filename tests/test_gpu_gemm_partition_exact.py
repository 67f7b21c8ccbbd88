"""The stem (csrc/conv_stem.hip), the 1x1 / stride 2 shortcut (csrc/conv1x1s2.hip) and the three products of the bottleneck
(csrc/bottleneck.hip) on the device, in EXACT arithmetic.  All of them are fp32 MFMA kernels, so there are no split pieces: with integer
operands every product and every partial sum is an integer below 2^24 (asserted), with one non-zero product per output the sum is that
product, and in both settings the float64 result of torch's operator cast to float32 is THE answer whatever the summation order --
torch.equal is the criterion.  Each stem / shortcut case of tests/gemm_partition_cases.py runs on its own grid (ops.set_reserved_cus,
restored afterwards): that makes ranges of several tiles (the register prefetch), ranges across images, the remainder loops of the two
reduce kernels, S = 1 and empty K ranges reachable with a handful of images; tests/test_gemm_partition_host.py asserts that the lists
contain every regime.

What BatchNorm makes of the bottleneck's products is not exact; it is held to the bars of tests/test_gpu_bottleneck.py against a float64
restatement, and dW to a derived rounding bound."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_plan_cases as C  # noqa: E402
import gemm_partition_cases as P  # noqa: E402
from test_gpu_conv_plan import grid, same  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = torch.nn.functional
STEM_W = (64, 3, 7, 7)


def gen(*seed):
    return torch.Generator().manual_seed(sum(s * 1000 ** i for i, s in enumerate(seed)))


def ints(shape, bound, *seed):
    return C.int_tensor(shape, bound, gen(*seed), DEV)


def arb(shape, *seed):
    return C.arbitrary_f32(shape, gen(*seed)).to(DEV)


def stem_fwd64(x, w):
    return F.conv2d(x.double(), w.double(), None, 2, 3)


def stem_wgrad64(gy, x):
    return torch.nn.grad.conv2d_weight(x.double(), STEM_W, gy.double(), 2, 3)


def twice(fn, what):
    """a weight gradient, run twice: bit-identical"""
    a, b = fn(), fn()
    assert torch.equal(a, b), what + ": two runs differ"
    return a


# ---- a. integer operands on every case -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.STEM_CASES, ids=P.stem_id)
def test_stem_integer_operands(case):
    from shapeclipper_amd import ops
    batch, G = case
    what = "stem " + P.stem_id(case)
    C.assert_exact_sum(P.STEM_TAPS, P.STEM_X_MAX, P.STEM_W_MAX)
    C.assert_exact_sum(batch * 112 * 112, P.STEM_X_MAX, P.STEM_GY_MAX)
    x, w = ints((batch, 3, 224, 224), P.STEM_X_MAX, batch, 1), ints(STEM_W, P.STEM_W_MAX, batch, 2)
    gy = ints((batch, 64, 112, 112), P.STEM_GY_MAX, batch, 3)
    with grid(G):
        same(ops.conv_stem_forward(x, w), stem_fwd64(x, w), what + " forward")
        same(twice(lambda: ops.conv_stem_backward_weight(gy, x), what), stem_wgrad64(gy, x), what + " weight gradient")


def ds_ref(hin, cin, cout, batch):
    """the three float64 operators of a shortcut shape"""
    fwd = lambda x, w: F.conv2d(x.double(), w.double(), None, 2)
    bd = lambda gy, w: torch.nn.grad.conv2d_input((batch, cin, hin, hin), w.double(), gy.double(), 2)
    wg = lambda gy, x: torch.nn.grad.conv2d_weight(x.double(), (cout, cin, 1, 1), gy.double(), 2)
    return fwd, bd, wg


@pytest.mark.parametrize("case", P.DS_CASES, ids=P.ds_id)
def test_shortcut_integer_operands(case):
    from shapeclipper_amd import ops
    hin, cin, cout, batch, G = case
    what = "1x1/2 " + P.ds_id(case)
    C.assert_exact_sum(max(cin, cout), max(P.DS_X_MAX, P.DS_GY_MAX), P.DS_W_MAX)
    C.assert_exact_sum(P.ds_npix(hin, batch), P.DS_X_MAX, P.DS_GY_MAX)
    x, w = ints((batch, cin, hin, hin), P.DS_X_MAX, hin, cin, 1), ints((cout, cin, 1, 1), P.DS_W_MAX, hin, cout, 2)
    gy = ints((batch, cout, hin // 2, hin // 2), P.DS_GY_MAX, hin, batch, 3)
    fwd, bd, wg = ds_ref(hin, cin, cout, batch)
    with grid(G):
        same(ops.conv1x1s2_forward(x, w), fwd(x, w), what + " forward")
        same(ops.conv1x1s2_backward_data(gy, w), bd(gy, w), what + " backward-data")
        same(twice(lambda: ops.conv1x1s2_backward_weight(gy, x), what), wg(gy, x), what + " weight gradient")


# ---- b. one product per output -----------------------------------------------------------------------------------------------------------------
def test_stem_forward_hot_input():
    """one hot pixel per image (corners, borders, interior pixels of every parity) under an arbitrary 24-bit filter, ranges of 18-19 tiles"""
    from shapeclipper_amd import ops
    batch, G = 5, 13
    pos = P.hot_positions(224)
    w = arb(STEM_W, 11)
    with grid(G):
        for shift in P.shifts(pos, batch):
            x = P.hot_maps(batch, 3, 224, pos, shift, own_channel=False).to(DEV)
            same(ops.conv_stem_forward(x, w), stem_fwd64(x, w), "stem forward, hot input, shift %d" % shift)


def test_stem_forward_one_hot_filter():
    """every output channel selects one (ci, ky, kx) of an arbitrary input; three runs visit all 147 taps: the o0 / o1 address
    arithmetic and the k = 147 pad (a zero filter row over the patch value of k = 146)"""
    from shapeclipper_amd import ops
    batch, G = 2, 9
    x = arb((batch, 3, 224, 224), 12)
    with grid(G):
        for run in range(P.STEM_FILTER_RUNS):
            w = P.stem_one_hot_filter(run).to(DEV)
            same(ops.conv_stem_forward(x, w), stem_fwd64(x, w), "stem forward, one-hot filter, run %d" % run)


def test_stem_weight_gradient_hot_gy():
    """one hot gy pixel per image, each in a channel of its own, with an arbitrary input"""
    from shapeclipper_amd import ops
    batch, G = 5, 13
    pos = P.hot_positions(112)
    x = arb((batch, 3, 224, 224), 13)
    with grid(G):
        for shift in P.shifts(pos, batch):
            gy = P.hot_maps(batch, 64, 112, pos, shift).to(DEV)
            same(ops.conv_stem_backward_weight(gy, x), stem_wgrad64(gy, x), "stem weight gradient, hot gy, shift %d" % shift)


def test_stem_weight_gradient_hot_input():
    """one hot input pixel per image, each in a channel of its own (so three images), with an arbitrary gy"""
    from shapeclipper_amd import ops
    batch, G = 3, 11
    pos = P.hot_positions(224)
    gy = arb((batch, 64, 112, 112), 14)
    with grid(G):
        for shift in P.shifts(pos, batch):
            x = P.hot_maps(batch, 3, 224, pos, shift).to(DEV)
            same(ops.conv_stem_backward_weight(gy, x), stem_wgrad64(gy, x), "stem weight gradient, hot input, shift %d" % shift)


@pytest.mark.parametrize("case", P.DS_CASES, ids=P.ds_id)
def test_shortcut_one_product(case):
    """a one-hot filter over arbitrary maps and hot maps under an arbitrary filter, for the three entry points"""
    from shapeclipper_amd import ops
    hin, cin, cout, batch, G = case
    what = "1x1/2 " + P.ds_id(case)
    x, gy = arb((batch, cin, hin, hin), hin, cin, 21), arb((batch, cout, hin // 2, hin // 2), hin, cout, 22)
    w = arb((cout, cin, 1, 1), hin, batch, 23)
    pos_x, pos_g = P.hot_positions(hin, 2), P.hot_positions(hin // 2)
    fwd, bd, wg = ds_ref(hin, cin, cout, batch)
    with grid(G):
        w_row, w_col = P.one_hot_matrix(cout, cin, "row").to(DEV), P.one_hot_matrix(cout, cin, "column").to(DEV)
        same(ops.conv1x1s2_forward(x, w_row), fwd(x, w_row), what + " forward, one-hot filter")
        same(ops.conv1x1s2_backward_data(gy, w_col), bd(gy, w_col), what + " backward-data, one-hot filter")
        for shift in P.shifts(pos_x, batch):
            xh = P.hot_maps(batch, cin, hin, pos_x, shift).to(DEV)
            same(ops.conv1x1s2_forward(xh, w), fwd(xh, w), what + " forward, hot input")
            same(ops.conv1x1s2_backward_weight(gy, xh), wg(gy, xh), what + " weight gradient, hot input")
        for shift in P.shifts(pos_g, batch):
            gh = P.hot_maps(batch, cout, hin // 2, pos_g, shift).to(DEV)
            same(ops.conv1x1s2_backward_data(gh, w), bd(gh, w), what + " backward-data, hot gy")
            same(ops.conv1x1s2_backward_weight(gh, x), wg(gh, x), what + " weight gradient, hot gy")


# ---- c. full overwrite ---------------------------------------------------------------------------------------------------------------------
def nan_like(shape):
    return torch.full(shape, float("nan"), device=DEV)


@pytest.mark.parametrize("case", [P.STEM_CASES[0], P.STEM_CASES[2]], ids=P.stem_id)
def test_stem_forward_overwrites_its_output(case):
    from shapeclipper_amd import _lib
    batch, G = case
    x, w = ints((batch, 3, 224, 224), P.STEM_X_MAX, batch, 31), ints(STEM_W, P.STEM_W_MAX, batch, 32)
    out = nan_like((batch, 64, 112, 112))
    with grid(G):
        _lib.check(_lib.load().sc_conv_stem_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(out), batch, _lib.stream()), "sc_conv_stem_forward")
        same(out, stem_fwd64(x, w), "stem " + P.stem_id(case) + " forward into NaN")


@pytest.mark.parametrize("case", [P.DS_CASES[0], P.DS_CASES[2]], ids=P.ds_id)
def test_shortcut_overwrites_its_outputs(case):
    """forward, and backward-data with its zeros at the odd rows and columns, into buffers full of NaN"""
    from shapeclipper_amd import _lib
    hin, cin, cout, batch, G = case
    what = "1x1/2 " + P.ds_id(case)
    x, w = ints((batch, cin, hin, hin), P.DS_X_MAX, hin, 33), ints((cout, cin, 1, 1), P.DS_W_MAX, hin, 34)
    gy = ints((batch, cout, hin // 2, hin // 2), P.DS_GY_MAX, hin, 35)
    fwd, bd, _ = ds_ref(hin, cin, cout, batch)
    out, gx = nan_like((batch, cout, hin // 2, hin // 2)), nan_like((batch, cin, hin, hin))
    lib = _lib.load()
    with grid(G):
        _lib.check(lib.sc_conv1x1s2_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(out), batch, cin, cout, hin, _lib.stream()), "sc_conv1x1s2_forward")
        _lib.check(lib.sc_conv1x1s2_backward_data(_lib.ptr(gy), _lib.ptr(w), _lib.ptr(gx), batch, cin, cout, hin, _lib.stream()),
                   "sc_conv1x1s2_backward_data")
        same(out, fwd(x, w), what + " forward into NaN")
        ref = bd(gy, w)
        assert float(ref[:, :, 1::2].abs().max()) == 0 and float(ref[:, :, :, 1::2].abs().max()) == 0
        same(gx, ref, what + " backward-data into NaN")


# ---- d. the stages of the bottleneck -------------------------------------------------------------------------------------------------------
def rel(a, b):
    return float((a.double() - b).abs().max()) / max(float(b.abs().max()), 1e-6)


def bl_stages(case, x_scale=P.BL_X_SCALE):
    """One linear + BatchNorm of the case forward (residual, ReLU) and backward twice (given g_out with the ReLU mask; g formed from the
    next layer, no ReLU, g_res wanted), and sc_linear_backward_data.  Asserts the exact products; returns what BatchNorm makes of them as
    {name: (error relative to the reference's largest element, bar)} and the dW errors as multiples of their bound."""
    from shapeclipper_amd import ops
    N, Cin, Cout, groups = case
    C.assert_exact_sum(Cin, max(P.BL_X_MAX, P.BL_G_MAX), P.BL_W_MAX, extra=P.BL_G_MAX)
    what = "bottleneck " + P.bl_id(case)
    x = ints((N, Cin), P.BL_X_MAX, N, Cout, 1) * x_scale                    # a power of two: as exact as the integers
    w = ints((Cout, Cin), P.BL_W_MAX, N, Cout, 2)
    g = gen(N, Cout, 3)
    gamma, beta = (torch.rand(Cout, generator=g) + 0.5).to(DEV), (torch.rand(Cout, generator=g) * 0.6 - 0.3).to(DEV)
    res = (torch.randn(N, Cout, generator=g) * 0.5).to(DEV)
    rm0, rv0 = (torch.rand(Cout, generator=g) * 0.4 - 0.2).to(DEV), (torch.rand(Cout, generator=g) + 0.5).to(DEV)
    rm, rv, tracked = rm0.clone(), rv0.clone(), torch.zeros((), dtype=torch.int64, device=DEV)
    out, y, stats = ops.linear_bn_forward(x, w, gamma, beta, res, rm, rv, tracked, True, P.BL_MOMENTUM, P.BL_EPS, True, groups)
    y64, out64, mean64, rstd64, rm64, rv64 = P.bl_reference(x.double(), w.double(), gamma.double(), beta.double(), res.double(), rm0.double(),
                                                            rv0.double(), groups, relu=True)
    same(y, y64, what + " y = x w^T")
    assert int(tracked) == groups
    soft = {"out": (rel(out, out64), 2e-5), "save_mean": (rel(stats[0], mean64), 1e-5), "save_rstd": (rel(stats[1], rstd64), 1e-5),
            "running_mean": (rel(rm, rm64), 1e-5), "running_var": (rel(rv, rv64), 1e-5)}
    dw_ratio = {}

    def check_bn_backward(tag, g64, got):
        gy, _, dw, dgamma, dbeta = got
        gy64, dgamma64, dbeta64 = P.bl_backward_reference(g64, y64, mean64, rstd64, gamma.double(), groups)
        soft.update({tag + " gy": (rel(gy, gy64), 5e-5), tag + " dgamma": (rel(dgamma, dgamma64), 5e-5), tag + " dbeta": (rel(dbeta, dbeta64), 5e-5)})
        # dW = gy^T x from the kernel's own gy: N products per element, one float32 rounding per addition
        dw64, bound = gy.double().T @ x.double(), P.gamma_n(N) * (gy.double().abs().T @ x.double().abs())
        dw_ratio[tag] = float(((dw.double() - dw64).abs() / bound.clamp_min(1e-300)).max())

    # given g_out, ReLU mask from `out`
    g_out = ints((N, Cout), P.BL_G_MAX, N, Cout, 4)
    got = ops.linear_bn_backward(g_out, None, None, None, out, y, stats, gamma, x, True, True, True, groups)
    g64 = g_out.double() * (out > 0)
    same(got[1], g64, what + " g_res = masked g_out")
    check_bn_backward("given", g64, got)
    # g = gy_next w_next + g_add, K = Cnext = Cin of the case (a multiple of 64)
    gy_next, w_next, g_add = ints((N, Cin), P.BL_G_MAX, N, Cout, 5), ints((Cin, Cout), P.BL_W_MAX, N, Cout, 6), ints((N, Cout), P.BL_G_MAX, N, Cout, 7)
    got = ops.linear_bn_backward(None, gy_next, w_next, g_add, out, y, stats, gamma, x, True, True, False, groups)
    g64 = gy_next.double() @ w_next.double() + g_add.double()
    same(got[1], g64, what + " g_res = gy_next w_next + g_add")
    check_bn_backward("formed", g64, got)
    # dx [N][Cout of the case] = gy [N][K] w [K][Cout of the case], K = Cin of the case
    same(ops.linear_backward_data(gy_next, w_next, None), gy_next.double() @ w_next.double(), what + " backward-data")
    same(ops.linear_backward_data(gy_next, w_next, g_add), g64, what + " backward-data + g_add")
    return soft, dw_ratio


@pytest.mark.parametrize("case", P.BL_CASES, ids=P.bl_id)
def test_bottleneck_stages(case):
    soft, dw_ratio = bl_stages(case)
    for name, (err, bar) in soft.items():
        print("%s %-20s %.2e of max (bar %.0e)" % (P.bl_id(case), name, err, bar))
    for name, ratio in dw_ratio.items():
        print("%s %-20s dW error %.3f of gamma_N sum|gy x|" % (P.bl_id(case), name, ratio))
    for name, (err, bar) in soft.items():
        assert err < bar, (name, err, bar)
    for name, ratio in dw_ratio.items():
        assert ratio <= 1.0, (name, ratio)


# ---- e. refusals: no kernel runs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [16, 48, 80])
def test_reduction_lengths_off_64_are_refused(K):
    """the four waves of gemm_rows take K / 4 each in steps of 16: K % 64 != 0 would read past the operands, so the entry points refuse"""
    from shapeclipper_amd import ops
    N, Cin, Cout, groups = 16, 64, 64, 1
    z = lambda *shape: torch.zeros(*shape, device=DEV)
    with pytest.raises(RuntimeError, match="sc_linear_backward_data"):
        ops.linear_backward_data(z(N, K), z(K, Cin), None)
    stats = torch.ones(2, groups, Cout, device=DEV)
    with pytest.raises(RuntimeError, match="sc_linear_bn_backward"):
        ops.linear_bn_backward(None, z(N, K), z(K, Cout), None, z(N, Cout), z(N, Cout), stats, z(Cout), z(N, Cin), True, True, False, groups)
    assert ops.linear_bn_supported(N, Cin, K, groups) and not ops.linear_bn_supported(N, K, Cout, groups)   # unchanged
