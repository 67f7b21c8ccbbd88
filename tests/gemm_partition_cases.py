"""Shared by tests/test_gemm_partition_host.py and tests/test_gpu_gemm_partition_exact.py: the work partitions of the stem
(csrc/conv_stem.hip) and of the 1x1 / stride 2 shortcut (csrc/conv1x1s2.hip) restated from their one-line formulas, the regimes a
(shape, grid) runs through, the GPU case lists, and the one-product operand patterns of the exact tests.  The bottleneck shapes
(csrc/bottleneck.hip), what they are chosen for and the float64 restatement of their BatchNorm are here too.  The tests take int_tensor,
assert_exact_sum and arbitrary_f32 from tests/conv_plan_cases.py; its one_hot_maps needs maps of side 4 and more channels than
images, which the shortcut's 1 x 1 maps and the stem's three input channels do not have: hot_maps below takes the positions."""
import torch

FULL = 0                                                # a case's grid: 0 = whatever the device has
FULL_GRIDS = range(64, 513)                             # a FULL case counts only for regimes it runs on every one of these grids


def cut(n, G):
    """[g * n // G, (g + 1) * n // G) for g < G: how both stem kernels and the 1x1 / 2 weight gradient cut n items over G owners"""
    return [(g * n // G, (g + 1) * n // G) for g in range(G)]


def _on(G, fn):
    """regimes of a case: fn(G) on its grid, or what fn gives on EVERY full grid"""
    if G != FULL:
        return fn(G)
    return set.intersection(*(fn(g) for g in FULL_GRIDS))


def _check_cut(ranges, n):
    assert ranges[0][0] == 0 and ranges[-1][1] == n and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])), "the ranges do not tile [0, n)"


# ---- the stem ------------------------------------------------------------------------------------------------------------------------------
ST_TILES, ST_STEPS = 49, 56                             # per image: 256-pixel tiles of the forward pass, two-row K-steps of the gradient
STEM_FWD_REGIMES = ("idle", "prefetch", "image_boundary", "mid_image_start", "first_tile_first", "first_tile_prefetched",
                    "last_tile_first", "last_tile_prefetched")
STEM_WGRAD_REGIMES = ("idle", "prefetch", "image_boundary", "reduce_rem0", "reduce_rem1", "reduce_rem2", "reduce_rem3")
STEM_CASES = ((1, FULL), (2, 9), (3, 10), (3, 11), (5, 13), (6, 8))       # (batch, G)
STEM_X_MAX, STEM_W_MAX, STEM_GY_MAX = 16, 4, 8


def stem_fwd_regimes(batch, G):
    def at(G):
        ranges = cut(ST_TILES * batch, G)
        _check_cut(ranges, ST_TILES * batch)
        r = set()
        for lo, hi in ranges:
            if lo == hi:
                r.add("idle")
                continue
            if hi - lo >= 2: r.add("prefetch")
            if lo // ST_TILES != (hi - 1) // ST_TILES: r.add("image_boundary")
            if lo % ST_TILES: r.add("mid_image_start")
            if lo % ST_TILES == 0: r.add("first_tile_first")                        # patch rows -3 .. -1 are padding
            if lo % ST_TILES == ST_TILES - 1: r.add("last_tile_first")              # patch rows 224 .. 226 are padding
            if any(t % ST_TILES == 0 for t in range(lo + 1, hi)): r.add("first_tile_prefetched")
            if any(t % ST_TILES == ST_TILES - 1 for t in range(lo + 1, hi)): r.add("last_tile_prefetched")
        return r
    return _on(G, at)


def stem_wgrad_regimes(batch, G):
    def at(G):
        ranges = cut(ST_STEPS * batch, G)
        _check_cut(ranges, ST_STEPS * batch)
        r = set()
        for lo, hi in ranges:
            if lo == hi:
                r.add("idle")
                continue
            if hi - lo >= 2: r.add("prefetch")
            if lo // ST_STEPS != (hi - 1) // ST_STEPS: r.add("image_boundary")
        # the reduce kernel's remainder loop adds the last G % 4 partial blocks: they must hold something for the loop to matter
        if all(lo < hi for lo, hi in ranges[G - G % 4:]): r.add("reduce_rem%d" % (G % 4))
        return r
    return _on(G, at)


def stem_id(c):
    return "B%d-G%s" % (c[0], c[1] or "full")


# ---- the 1x1 / stride 2 shortcut -----------------------------------------------------------------------------------------------------------
DS_GEMM_REGIMES = ("npix_below_tile", "ragged_last_tile", "npix_multiple_of_tile", "tile_spans_images", "two_channel_tiles", "k64", "k_ge_128")
DS_WGRAD_REGIMES = ("s_one", "s_even", "s_odd", "empty_ranges", "range_of_two_steps", "ragged_last_step", "step_spans_images")
DS_CASES = (                                            # (hin, cin, cout, batch, G)
    (2, 64, 64, 1, FULL),
    (6, 64, 128, 3, 9),
    (14, 128, 128, 5, 13),
    (14, 128, 192, 3, 8),                               # six blocks on eight workgroups: S = 1
    (28, 64, 64, 2, 11),
    (8, 64, 64, 8, 10),                                 # npix = 128
)
DS_X_MAX, DS_W_MAX, DS_GY_MAX = 16, 4, 16


def ds_npix(hin, batch):
    return batch * (hin // 2) ** 2


def ds_gemm_regimes(hin, cin, cout, batch, mode):
    """conv1x1s2_gemm_kernel: mode "forward" (M = cout, K = cin) or "backward_data" (M = cin, K = cout); 128-pixel tiles, no grid in it"""
    M, K = (cout, cin) if mode == "forward" else (cin, cout)
    npix, hwo = ds_npix(hin, batch), (hin // 2) ** 2
    tiles = (npix + 127) // 128
    r = set()
    if npix < 128: r.add("npix_below_tile")
    if tiles >= 2 and npix % 128: r.add("ragged_last_tile")
    if npix % 128 == 0: r.add("npix_multiple_of_tile")
    if any(128 * t // hwo != (min(128 * t + 128, npix) - 1) // hwo for t in range(tiles)): r.add("tile_spans_images")
    if M >= 128: r.add("two_channel_tiles")
    if K == 64: r.add("k64")
    if K >= 128: r.add("k_ge_128")
    return r


def ds_splits(cin, cout, G):
    return max(1, G // ((cin // 64) * (cout // 64)))


def ds_wgrad_regimes(hin, cin, cout, batch, G):
    def at(G):
        npix, hwo = ds_npix(hin, batch), (hin // 2) ** 2
        S, ksteps = ds_splits(cin, cout, G), (npix + 63) // 64
        ranges = cut(ksteps, S)
        _check_cut(ranges, ksteps)
        r = set()
        if S == 1: r.add("s_one")
        if S > 1 and S % 2 == 0: r.add("s_even")
        if S >= 3 and S % 2 and ranges[-1][0] < ranges[-1][1]: r.add("s_odd")   # the reduce kernel's single-element tail, with work in it
        if S > ksteps and any(lo == hi for lo, hi in ranges): r.add("empty_ranges")
        if any(hi - lo >= 2 for lo, hi in ranges): r.add("range_of_two_steps")
        if npix % 64: r.add("ragged_last_step")
        if any(64 * k // hwo != (min(64 * k + 64, npix) - 1) // hwo for k in range(ksteps)): r.add("step_spans_images")
        return r
    return _on(G, at)


def ds_id(c):
    return "%dx%d-%d>%d-B%d-G%s" % (c[0], c[0], c[1], c[2], c[3], c[4] or "full")


# ---- one-product operand patterns ----------------------------------------------------------------------------------------------------------
def hot_positions(side, step=1):
    """(y, x) of the hot pixel per image, in turn: the four corners, two mid-border pixels, interior pixels of the four (row, column)
    parities -- as far as a map of this side has them (conv_plan_cases.hot_pixels needs a side of 4; the shortcut's maps go down to 1 x 1).
    step = 2: the same on the even positions a stride-2 1x1 convolution reads, then one odd position that it must not read."""
    n = (side - 1) // step                              # last position, in units of step
    e = n // 2 - n // 2 % 2
    o = min(e + 1, n)
    units = [(0, 0), (n, n), (0, n), (n, 0), (e, n), (0, o), (e, e), (o, e), (o, o), (e, o)]
    pos = list(dict.fromkeys((y * step, x * step) for y, x in units))
    return pos + [(1, 1)] if step == 2 else pos


def hot_maps(batch, channels, side, positions, shift=0, value=1.0, own_channel=True):
    """one pixel of one channel per image is `value`: image b has positions[(b + shift) % len], in channel 5 + 11 (b + shift) (both lane
    halves, several K-steps).  own_channel: no two images share a channel, as a sum over images (a weight gradient) needs it."""
    x = torch.zeros(batch, channels, side, side)
    chans = [(5 + 11 * (b + shift)) % channels for b in range(batch)]
    assert len(set(chans)) == batch or not own_channel
    for b in range(batch):
        y, xx = positions[(b + shift) % len(positions)]
        x[b, chans[b], y, xx] = value
    return x


def shifts(positions, batch):
    """the shifts with which hot_maps puts every position into some image"""
    return range(0, len(positions), batch)


STEM_TAPS = 147
STEM_FILTER_RUNS = 3                                    # 3 x 64 output channels >= 147 taps


def stem_one_hot_filter(run):
    """w[co, tap(co)] = 1 with tap = (ci, ky, kx) flattened = (co + 64 run) % 147: runs 0..2 visit all 147 taps"""
    w = torch.zeros(64, STEM_TAPS)
    co = torch.arange(64)
    w[co, (co + 64 * run) % STEM_TAPS] = 1.0
    return w.view(64, 3, 7, 7)


def one_hot_matrix(cout, cin, per):
    """a [cout][cin] 1x1 filter with one 1 per row (per = "row": one product per forward output) or per column ("column": one product per
    backward-data output); the other index runs over both lane halves and every 16-wide K-step"""
    w = torch.zeros(cout, cin)
    if per == "row":
        co = torch.arange(cout)
        w[co, (co * 5 + co // 9) % cin] = 1.0
    else:
        ci = torch.arange(cin)
        w[(ci * 5 + ci // 9) % cout, ci] = 1.0
    return w.view(cout, cin, 1, 1)


# ---- the bottleneck ------------------------------------------------------------------------------------------------------------------------
# (N, Cin, Cout, groups).  A lane of the kernels holds rows 16 t + 4 kg .. + 3 of a 16-row tile.
BL_CASES = ((20, 64, 16, 2), (6, 64, 48, 3), (100, 128, 80, 4), (128, 64, 64, 1), (2, 64, 64, 1))
BL_REGIMES = ("group_boundary_inside_a_lane", "ragged_last_row_tile", "cout_not_multiple_of_64", "all_eight_row_tiles", "one_row_tile", "k_ge_128")
BL_X_MAX, BL_W_MAX, BL_G_MAX = 8, 4, 8
# x = integers * 2^-14: every product and sum is exact as with integers, and the batch variance of y = x w^T (|y| of a few 2^-8) comes
# to lie next to eps = 1e-5.  With integer y and two rows per group the variance is 1e4 .. 1e9 eps, and gy -- analytically
# O(eps / var) of g -- is the difference of two float32 numbers that agree in all but their last bits: no float32 BatchNorm meets a
# relative bar there, whatever its code.
BL_X_SCALE = 2.0 ** -14
BL_EPS, BL_MOMENTUM = 1e-5, 0.1


def bl_regimes(N, Cin, Cout, groups):
    ng = N // groups
    r = set()
    if any((g * ng) % 4 for g in range(1, groups)): r.add("group_boundary_inside_a_lane")
    if N % 16: r.add("ragged_last_row_tile")
    if Cout % 64: r.add("cout_not_multiple_of_64")
    if N > 112: r.add("all_eight_row_tiles")
    if N <= 16: r.add("one_row_tile")
    if Cin >= 128: r.add("k_ge_128")
    return r


def bl_id(c):
    return "N%d-%d>%d-g%d" % c


def bl_reference(x, w, gamma, beta, res, run_mean, run_var, groups, relu, eps=BL_EPS, momentum=BL_MOMENTUM):
    """sc_linear_bn_forward in training mode, restated in float64 (all arguments float64): per-group statistics, the biased variance
    under the square root, the unbiased one into running_var, one momentum update per group in order.
    -> y, out, mean [G][Cout], rstd [G][Cout], run_mean, run_var"""
    N, ng = x.shape[0], x.shape[0] // groups
    y = x @ w.T
    yg = y.view(groups, ng, -1)
    mean, var = yg.mean(1), yg.var(1, unbiased=False)
    rstd = (var + eps).rsqrt()
    out = ((yg - mean[:, None]) * rstd[:, None]).reshape(N, -1) * gamma + beta
    if res is not None:
        out = out + res
    if relu:
        out = out.clamp_min(0)
    run_mean, run_var = run_mean.clone(), run_var.clone()
    for g in range(groups):
        run_mean = (1 - momentum) * run_mean + momentum * mean[g]
        run_var = (1 - momentum) * run_var + momentum * (var[g] * ng / (ng - 1) if ng > 1 else var[g])
    return y, out, mean, rstd, run_mean, run_var


def bl_backward_reference(g, y, mean, rstd, gamma, groups):
    """BatchNorm backward of sc_linear_bn_backward in training mode, float64: g [N][Cout] the (masked) incoming gradient
    -> gy, dgamma, dbeta"""
    N, ng = y.shape[0], y.shape[0] // groups
    xh = (y.view(groups, ng, -1) - mean[:, None]) * rstd[:, None]
    gg = g.view(groups, ng, -1)
    sb, sg = gg.sum(1, keepdim=True), (gg * xh).sum(1, keepdim=True)
    gy = gamma * rstd[:, None] * (gg - sb / ng - xh * sg / ng)
    return gy.reshape(N, -1), sg.sum((0, 1)), sb.sum((0, 1))


def gamma_n(n):
    """the bound of n float32 roundings in a row, (1 + 2^-24)^n - 1 <= n u / (1 - n u)"""
    u = 2.0 ** -24
    return n * u / (1 - n * u)
