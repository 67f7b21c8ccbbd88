"""The work partitions of the stem (csrc/conv_stem.hip), of the 1x1 / stride 2 shortcut (csrc/conv1x1s2.hip) and the row / channel
tiling of the bottleneck (csrc/bottleneck.hip) on the host: no GPU.  The partitions are one-line formulas, restated in
tests/gemm_partition_cases.py; checked here: the GPU case lists of tests/test_gpu_gemm_partition_exact.py contain every regime of
every kernel (a case on the full grid counts only for what it runs on every grid of 64..512); the integer operands keep every
partial sum exact; and the one-product patterns give float64 results that are float32 numbers and visit what they are meant to."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_plan_cases as C  # noqa: E402
import gemm_partition_cases as P  # noqa: E402


def _covered(name, regimes, got):
    for case, r in got.items():
        print("%-10s %-28s %s" % (name, case, " ".join(sorted(r))))
        assert r <= set(regimes), (case, sorted(r - set(regimes)))
    missing = set(regimes) - set().union(*got.values())
    assert not missing, (name, sorted(missing))


def _grids_ok(grids):
    assert all(G == P.FULL or 8 <= G < 64 for G in grids), "a case names its grid; the full grid is not named"
    assert any(G == P.FULL for G in grids), "one case stays on the full grid"


def test_stem_cases_contain_every_regime():
    _grids_ok([G for _, G in P.STEM_CASES])
    _covered("stem fwd", P.STEM_FWD_REGIMES, {P.stem_id(c): P.stem_fwd_regimes(*c) for c in P.STEM_CASES})
    _covered("stem wgrad", P.STEM_WGRAD_REGIMES, {P.stem_id(c): P.stem_wgrad_regimes(*c) for c in P.STEM_CASES})


def test_shortcut_cases_contain_every_regime():
    _grids_ok([c[4] for c in P.DS_CASES])
    for mode in ("forward", "backward_data"):
        _covered("1x1/2 " + mode, P.DS_GEMM_REGIMES, {P.ds_id(c): P.ds_gemm_regimes(*c[:4], mode) for c in P.DS_CASES})
    _covered("1x1/2 wgrad", P.DS_WGRAD_REGIMES, {P.ds_id(c): P.ds_wgrad_regimes(*c) for c in P.DS_CASES})


def test_bottleneck_cases_contain_every_regime():
    from shapeclipper_amd import _lib
    lib = _lib.load()                                                        # (sc_linear_bn_supported asks no device)
    for N, Cin, Cout, groups in P.BL_CASES:
        assert lib.sc_linear_bn_supported(N, Cin, Cout, groups) == 1 and Cin % 64 == 0      # Cin is the K of both backward products here
    _covered("bottleneck", P.BL_REGIMES, {P.bl_id(c): P.bl_regimes(*c) for c in P.BL_CASES})


def test_a_full_case_claims_only_what_every_grid_runs():
    """On 255, 256 or 304 workgroups a case gives at least what it is counted for; a regime that depends on the grid (the parity of S,
    G % 4) is never counted for a full case."""
    for batch, G in P.STEM_CASES:
        if G == P.FULL:
            claimed = P.stem_wgrad_regimes(batch, G)
            assert not any(r.startswith("reduce_rem") for r in claimed)
            for g in (64, 255, 256, 304):
                assert claimed <= P.stem_wgrad_regimes(batch, g) and P.stem_fwd_regimes(batch, G) <= P.stem_fwd_regimes(batch, g)
    for c in P.DS_CASES:
        if c[4] == P.FULL:
            claimed = P.ds_wgrad_regimes(*c)
            assert not claimed & {"s_one", "s_even", "s_odd"}
            for g in (64, 255, 256, 304):
                assert claimed <= P.ds_wgrad_regimes(*c[:4], g)


def test_cut_counts_every_item_once():
    for n in (1, 2, 7, 49, 56, 98, 147, 336):
        for G in list(range(1, 41)) + [255, 256, 304]:
            ranges = P.cut(n, G)
            seen = [i for lo, hi in ranges for i in range(lo, hi)]
            assert seen == list(range(n)) and max(hi - lo for lo, hi in ranges) - min(hi - lo for lo, hi in ranges) <= 1


def test_integer_sums_stay_exact():
    """the bounds the GPU tests draw their integers from, at the largest case of each kernel"""
    batch = max(b for b, _ in P.STEM_CASES)
    C.assert_exact_sum(P.STEM_TAPS, P.STEM_X_MAX, P.STEM_W_MAX)
    C.assert_exact_sum(batch * 112 * 112, P.STEM_X_MAX, P.STEM_GY_MAX)
    for hin, cin, cout, b, _ in P.DS_CASES:
        C.assert_exact_sum(max(cin, cout), P.DS_X_MAX, P.DS_W_MAX)
        C.assert_exact_sum(P.ds_npix(hin, b), P.DS_X_MAX, P.DS_GY_MAX)
    for N, Cin, Cout, _ in P.BL_CASES:
        C.assert_exact_sum(Cin, max(P.BL_X_MAX, P.BL_G_MAX), P.BL_W_MAX, extra=P.BL_G_MAX)
    with pytest.raises(AssertionError):
        C.assert_exact_sum(batch * 112 * 112, 16, 16)


def test_hot_positions_and_filters_visit_what_they_should():
    for side in (224, 112):
        pos = P.hot_positions(side)
        assert len(set(pos)) == len(pos) == 10 and all(0 <= y < side and 0 <= x < side for y, x in pos)
        assert {(0, 0), (0, side - 1), (side - 1, 0), (side - 1, side - 1)} <= set(pos)
        interior = [(y, x) for y, x in pos if 3 <= y < side - 3 and 3 <= x < side - 3]
        assert {(y % 2, x % 2) for y, x in interior} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert any(x == side - 1 and 3 <= y < side - 3 for y, x in pos) and any(y == 0 and 3 <= x < side - 3 for y, x in pos)
    for hin, *_ in P.DS_CASES:
        for side, step in ((hin, 2), (hin // 2, 1)):
            pos = P.hot_positions(side, step)
            assert len(set(pos)) == len(pos) and all(0 <= y < side and 0 <= x < side for y, x in pos)
            assert pos[0] == (0, 0) and all(y % step == 0 and x % step == 0 for y, x in pos[:len(pos) - (step == 2)])
            assert step == 1 or pos[-1] == (1, 1)                                # the one position a stride-2 read must skip
    taps = set()
    for run in range(P.STEM_FILTER_RUNS):
        w = P.stem_one_hot_filter(run)
        assert w.shape == (64, 3, 7, 7) and (w.flatten(1).sum(1) == 1).all()
        taps |= set(w.flatten(1).argmax(1).tolist())
    assert taps == set(range(P.STEM_TAPS))
    for cout, cin in ((64, 64), (128, 64), (64, 128), (192, 128)):
        assert (P.one_hot_matrix(cout, cin, "row").flatten(1).sum(1) == 1).all()
        assert (P.one_hot_matrix(cout, cin, "column").flatten(1).sum(0) == 1).all()
    x = P.hot_maps(5, 3 * 7, 8, P.hot_positions(8), shift=5)
    assert x.shape == (5, 21, 8, 8) and (x.flatten(2).sum(2).sum(1) == 1).all() and (x.sum((0, 2, 3)) <= 1).all()
    assert list(P.shifts(P.hot_positions(224), 5)) == [0, 5] and list(P.shifts(P.hot_positions(224), 3)) == [0, 3, 6, 9]


def _f32(t64):
    return torch.equal(t64.float().double(), t64)


def test_one_product_references_are_float32():
    """What the GPU tests rely on: with one non-zero product per output the float64 result is a float32 tensor -- shown on the stem
    patterns at batch 1 and on the shortcut patterns of one case; with TWO hot images in one channel it is not (the premise is not empty)."""
    gen = torch.Generator().manual_seed(1)
    pos = P.hot_positions(224)
    x = P.hot_maps(1, 3, 224, pos, shift=8)
    w = C.arbitrary_f32((64, 3, 7, 7), gen)
    y64 = torch.nn.functional.conv2d(x.double(), w.double(), None, 2, 3)
    assert _f32(y64) and int((y64 != 0).sum()) == 64 * 16                   # an interior odd / odd pixel meets 4 x 4 taps
    xa = C.arbitrary_f32((1, 3, 224, 224), gen)
    assert _f32(torch.nn.functional.conv2d(xa.double(), P.stem_one_hot_filter(2).double(), None, 2, 3))
    gy = C.arbitrary_f32((1, 64, 112, 112), gen)
    assert _f32(torch.nn.grad.conv2d_weight(x.double(), (64, 3, 7, 7), gy.double(), 2, 3))
    both = P.hot_maps(1, 3, 224, pos, shift=2) + P.hot_maps(1, 3, 224, pos, shift=5)     # one channel, rows and columns of one parity
    two = torch.nn.grad.conv2d_weight(both.double(), (64, 3, 7, 7), gy.double(), 2, 3)
    assert bool((both.sum((0, 2, 3)) == 2).any()) and not _f32(two)
    hin, cin, cout, batch, _ = P.DS_CASES[2]
    xm, gm = C.arbitrary_f32((batch, cin, hin, hin), gen), C.arbitrary_f32((batch, cout, hin // 2, hin // 2), gen)
    wa = C.arbitrary_f32((cout, cin, 1, 1), gen)
    xh = P.hot_maps(batch, cin, hin, P.hot_positions(hin, 2))
    gh = P.hot_maps(batch, cout, hin // 2, P.hot_positions(hin // 2))
    conv = torch.nn.functional.conv2d
    assert _f32(conv(xm.double(), P.one_hot_matrix(cout, cin, "row").double(), None, 2)) and _f32(conv(xh.double(), wa.double(), None, 2))
    bd = lambda g, w: torch.nn.grad.conv2d_input((batch, cin, hin, hin), w.double(), g.double(), 2)
    assert _f32(bd(gm, P.one_hot_matrix(cout, cin, "column"))) and _f32(bd(gh, wa))
    assert not _f32(bd(gm, wa))
    wg = lambda g, x_: torch.nn.grad.conv2d_weight(x_.double(), (cout, cin, 1, 1), g.double(), 2)
    assert _f32(wg(gh, xm)) and _f32(wg(gm, xh)) and not _f32(wg(gm, xm))


def test_bottleneck_reference_is_the_stock_batchnorm():
    """P.bl_reference / P.bl_backward_reference against torch's own float64 batch_norm and autograd, per group"""
    torch.manual_seed(3)
    N, Cin, Cout, groups = 12, 8, 5, 3
    x, w = torch.randn(N, Cin, dtype=torch.float64), torch.randn(Cout, Cin, dtype=torch.float64)
    gamma, beta = torch.rand(Cout, dtype=torch.float64) + 0.5, torch.randn(Cout, dtype=torch.float64)
    rm, rv = torch.randn(Cout, dtype=torch.float64), torch.rand(Cout, dtype=torch.float64) + 0.5
    res, cot = torch.randn(N, Cout, dtype=torch.float64), torch.randn(N, Cout, dtype=torch.float64)
    y, out, mean, rstd, rm1, rv1 = P.bl_reference(x, w, gamma, beta, res, rm, rv, groups, relu=False)
    yl = (x @ w.T).requires_grad_(True)
    rm2, rv2 = rm.clone(), rv.clone()
    stock = torch.cat([torch.nn.functional.batch_norm(v, rm2, rv2, gamma, beta, True, P.BL_MOMENTUM, P.BL_EPS) for v in yl.chunk(groups)]) + res
    close = lambda a, b: float((a - b).abs().max()) < 1e-12 * max(1.0, float(b.abs().max()))
    assert close(out, stock.detach()) and close(rm1, rm2) and close(rv1, rv2) and torch.equal(y, yl.detach())
    gamma_l = gamma.clone().requires_grad_(True)
    stock = torch.cat([torch.nn.functional.batch_norm(v, None, None, gamma_l, beta, True, P.BL_MOMENTUM, P.BL_EPS) for v in yl.chunk(groups)])
    stock.backward(cot)
    gy, dgamma, dbeta = P.bl_backward_reference(cot, y, mean, rstd, gamma, groups)
    assert close(gy, yl.grad) and close(dgamma, gamma_l.grad) and close(dbeta, cot.sum(0))
    assert abs(P.gamma_n(128) - 128 * 2.0 ** -24) < 1e-10
