"""Shared by tests/test_conv_plan_host.py, tests/test_gpu_conv_plan.py and tests/test_gpu_conv_split_exact.py: the work partition of the
3x3 convolution launches (conv3x3_kernel / conv3x3_fixup_kernel in csrc/conv3x3.hip) as sc_conv3x3_plan reports it, a Python replay of
what the two kernels do with it, the regimes of a plan, the GPU case list, and the operand builders (integer operands for the
partition sweep; one-product patterns and a torch emulation of the three-piece bf16 split for the exact tests of the six products).

A product is named (p, q) = piece p of the input (or of gy) times piece q of the filter (weight gradient: piece p of x, q of gy)."""
import ctypes
import functools

import numpy as np
import torch

FAMILIES = ("fp32", "split", "s2fwd", "s2bd")          # sc_conv3x3_plan's family 0..3
FAM = {name: i for i, name in enumerate(FAMILIES)}
PLAN_FIELDS = ("tiles", "nk", "rounds", "tail_tiles", "per_wg", "PT", "CT", "ov2", "G", "table")
PRODUCTS = ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
def plan(family, side, batch, cin, cout, cus, equal=False):
    """sc_conv3x3_plan as a dict (PLAN_FIELDS, "spans" = list of G + 1 starts), or the refusal's status.  cus > 0: no device call."""
    from shapeclipper_amd import _lib
    lib = _lib.load()
    head = (ctypes.c_int * 10)(*([-1] * 10))
    args = (FAM[family], side, batch, cin, cout, cus, int(equal))
    rc = lib.sc_conv3x3_plan(*args, head, None)
    if rc:
        assert list(head) == [-1] * 10, "a refusal wrote a plan"
        return rc
    spans = (ctypes.c_int * (head[8] + 1))()
    assert lib.sc_conv3x3_plan(*args, head, spans) == 0
    p = dict(zip(PLAN_FIELDS, head))
    p["spans"] = list(spans)
    return p


def out_pixels(family, side, batch):
    """flat output pixels the tiles cover (stride-2 backward-data: pixels of the gradient map, every parity phase has them all)"""
    return batch * (side * side if family in ("fp32", "split") else (side // 2) ** 2)


def tile_channels(family, cin, cout):
    """channels the tiles divide: the convolution's output channels (stride-2 backward-data: the forward input channels)"""
    return cin if family == "s2bd" else cout


def reduce_channels(family, cin, cout):
    return cout if family == "s2bd" else cin


def expected_head(family, side, batch, cin, cout, p):
    """tiles and nk of plan p restated from the shapes (PT, CT taken from the plan)"""
    cdiv = lambda a, b: (a + b - 1) // b
    tiles = cdiv(out_pixels(family, side, batch), p["PT"]) * cdiv(tile_channels(family, cin, cout), p["CT"]) * (4 if family == "s2bd" else 1)
    nk = reduce_channels(family, cin, cout) // 8
    return tiles, (nk + 1) & ~1 if family == "split" else nk


def greedy_cut(tail_tiles, nk, G, ov2):
    """The span table restated: a span costs 2 * K-steps + ov2 * tiles touched; the greedy cut (every span as long as the bound, nk steps
    and the end allow, at least one step) at the smallest bound with which G spans cover all tail_tiles * nk steps."""
    total = tail_tiles * nk

    def build(bound):
        U, pos = [], 0
        for _ in range(G):
            U.append(pos)
            end = pos
            while end < total and end - pos < nk:
                items = end // nk - pos // nk + 1                      # tiles touched by [pos, end + 1)
                if end > pos and 2 * (end + 1 - pos) + ov2 * items > bound:
                    break
                end += 1
            pos = end
        return U + [total], pos >= total

    lo = 2 * ((total + G - 1) // G)
    hi = lo + 4 * ov2 + 4
    while not build(hi)[1]:
        hi += 2 * nk
    while lo < hi:
        mid = (lo + hi) // 2
        if build(mid)[1]:
            hi = mid
        else:
            lo = mid + 1
    return build(hi)[0]


@functools.lru_cache(maxsize=None)
def gperm(G):
    """tile of a whole round that workgroup g takes (workgroup g runs on XCD g % 8; every XCD gets a contiguous range)"""
    xq, xr = G >> 3, G & 7
    return tuple((x * (xq + 1) if x < xr else xr * (xq + 1) + (x - xr) * xq) + (g >> 3) for g in range(G) for x in (g & 7,))


def span_at(p, g):
    """conv_span_at: from the table, or computed for equal spans"""
    return p["spans"][g] if p["table"] else min(g * p["per_wg"], p["tail_tiles"] * p["nk"])


def span_owner(p, u):
    """conv_span_owner: the device's binary search over the table, or the division of the equal-span fallback"""
    if not p["table"]:
        return u // p["per_wg"]
    lo, hi = 0, p["G"] - 1
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if p["spans"][mid] <= u:
            lo = mid
        else:
            hi = mid - 1
    return lo


def kernel_items(p, g):
    """The items of conv3x3_kernel's workgroup g: (item, tile, kb0, kb1) in item order (the device order differs, the set does not)."""
    nk, G, rounds = p["nk"], p["G"], p["rounds"]
    perm = gperm(G)
    lo, hi = span_at(p, g), span_at(p, g + 1)
    items = [(r, r * G + perm[g], 0, nk) for r in range(rounds)]
    if lo < hi:
        t = lo // nk
        items.append((rounds, rounds * G + t, lo - t * nk, min(nk, hi - t * nk)))
        t += 1
        if t * nk < hi:
            items.append((rounds + 1, rounds * G + t, 0, hi - t * nk))
    return items


def replay(p):
    """Replays conv3x3_kernel and conv3x3_fixup_kernel over plan p and asserts that every K-step of every tile is counted exactly once.
    Returns the partial items [(g, slot, tile, kb0, kb1)] and the set of tail tiles stored whole (regimes() reads both)."""
    nk, G, rounds, tail, tiles = p["nk"], p["G"], p["rounds"], p["tail_tiles"], p["tiles"]
    assert rounds == tiles // G and tail == tiles - rounds * G and p["per_wg"] == (tail * nk + G - 1) // G and len(p["spans"]) == G + 1
    assert sorted(gperm(G)) == list(range(G)), "gperm is not a permutation"
    U = [span_at(p, g) for g in range(G + 1)]
    assert U[0] == 0 and U[G] == tail * nk and all(a <= b for a, b in zip(U, U[1:])), "span starts"
    assert U == p["spans"], "the exported span starts are not what conv_span_at gives the kernels"
    stored = np.zeros(tiles, dtype=np.int64)                            # whole-tile stores of conv3x3_kernel
    partial = {}                                                        # (g, slot) -> (tile, kb0, kb1)
    for g in range(G):
        lo, hi = U[g], U[g + 1]
        assert hi - lo <= nk, "a span longer than a tile"
        if hi > lo:
            assert (hi - 1) // nk - lo // nk <= 1, "a span over three tiles"
        for item, tile, kb0, kb1 in kernel_items(p, g):
            assert 0 <= tile < tiles and 0 <= kb0 < kb1 <= nk, (g, item, tile, kb0, kb1)
            if kb0 == 0 and kb1 == nk:
                stored[tile] += 1
            else:
                assert item >= rounds
                partial[(g, item - rounds)] = (tile, kb0, kb1)
    assert (stored[:rounds * G] == 1).all(), "a tile of the whole rounds is not stored exactly once"
    whole_tail = set()
    for t in range(tail):                                               # one fix-up workgroup row per tail tile
        tile = rounds * G + t
        u0, u1 = t * nk, t * nk + nk
        g_first, g_last = span_owner(p, u0), span_owner(p, u1 - 1)
        if g_first == g_last and span_at(p, g_first) == u0 and span_at(p, g_first + 1) == u1:
            assert stored[tile] == 1, "the fix-up skips tile %d, which nobody stored" % tile
            whole_tail.add(t)
            continue
        assert stored[tile] == 0, "tile %d is stored whole and summed" % tile
        k = 0
        for g in range(g_first, g_last + 1):
            which = 0 if span_at(p, g) // nk == t else 1
            assert (g, which) in partial, "the fix-up reads slot %d of workgroup %d, which was not written" % (which, g)
            ptile, kb0, kb1 = partial.pop((g, which))
            assert ptile == tile and kb0 == k, ("partials of tile %d do not abut in K order" % tile, g, which, ptile, kb0, kb1)
            k = kb1
        assert k == nk, "the partials of tile %d end at K-step %d of %d" % (tile, k, nk)
    assert not partial, "partial tiles nobody reads: %r" % sorted(partial)
    return [(g, it - rounds, tile, kb0, kb1) for g in range(G) for it, tile, kb0, kb1 in kernel_items(p, g)
            if it >= rounds and not (kb0 == 0 and kb1 == nk)], whole_tail


# ---- regimes ---------------------------------------------------------------------------------------------------------------------------
REGIMES = ("whole_rounds_only", "rounds_and_tail", "two_rounds", "xcd_remainder", "idle_workgroups", "crossing", "crossing_odd_start",
           "odd_start_single", "odd_start_long", "even_start_single", "even_end_long", "tail_all_whole", "ragged_pixels", "ragged_channels")


def regimes(family, side, batch, cin, cout, p):
    """The regimes (names of REGIMES) that plan p of this shape runs through.  The parity regimes are about one item of a workgroup: the
    K-steps [kb0, kb1) it computes of one tile -- what the PAIRED instance's re-staging of the even partner depends on."""
    parts, whole_tail = replay(p)
    nk, G, tail = p["nk"], p["G"], p["tail_tiles"]
    U = [span_at(p, g) for g in range(G + 1)]
    crossing = [g for g in range(G) if U[g] < U[g + 1] and U[g] // nk != (U[g + 1] - 1) // nk]
    segs = [(kb0, kb1) for _, _, _, kb0, kb1 in parts]
    r = set()
    if p["rounds"] >= 1 and tail == 0: r.add("whole_rounds_only")
    if p["rounds"] >= 1 and tail > 0: r.add("rounds_and_tail")
    if p["rounds"] >= 2: r.add("two_rounds")
    if p["rounds"] >= 1 and G % 8: r.add("xcd_remainder")
    if tail > 0 and any(U[g] == U[g + 1] for g in range(G)): r.add("idle_workgroups")
    if crossing: r.add("crossing")
    if any(U[g] % nk % 2 for g in crossing): r.add("crossing_odd_start")
    if any(a % 2 and b - a == 1 for a, b in segs): r.add("odd_start_single")
    if any(a % 2 and b - a >= 2 for a, b in segs): r.add("odd_start_long")
    if any(a % 2 == 0 and b - a == 1 for a, b in segs): r.add("even_start_single")
    if any(b % 2 and b - a >= 2 for a, b in segs): r.add("even_end_long")          # last step b - 1 even; a partial item with b odd has b < nk or nk odd
    if tail > 0 and len(whole_tail) == tail: r.add("tail_all_whole")
    if out_pixels(family, side, batch) % p["PT"]: r.add("ragged_pixels")
    if tile_channels(family, cin, cout) % p["CT"]: r.add("ragged_channels")
    return r


# The GPU sweep: (family, side, cin, cout, batch, G).  side / cin / cout as the entry point takes them (stride 2: side of the forward
# input, channels of the forward convolution).  G: grid the case runs on (ops.set_reserved_cus(device CUs - G)); 0 = the full grid.
# tests/test_conv_plan_host.py asserts, from the exported plans, that every family's rows together contain every regime of REGIMES
# but those of IMPOSSIBLE.
GPU_CASES = (
    ("split", 14, 24, 64, 34, 9),
    ("split", 7, 64, 72, 37, 8),
    ("split", 7, 24, 64, 1, 8),
    ("split", 7, 24, 64, 27, 8),
    ("split", 14, 64, 64, 2, 0),
    ("fp32", 14, 128, 64, 32, 11),
    ("fp32", 7, 24, 64, 19, 8),
    ("fp32", 7, 24, 64, 11, 8),
    ("fp32", 7, 24, 64, 1, 8),
    ("fp32", 14, 64, 64, 2, 0),
    ("s2fwd", 14, 32, 72, 32, 9),
    ("s2fwd", 14, 8, 136, 27, 8),
    ("s2fwd", 14, 8, 136, 11, 9),
    ("s2fwd", 14, 64, 64, 2, 0),
    ("s2bd", 14, 72, 64, 27, 13),
    ("s2bd", 14, 8, 64, 6, 8),
    ("s2bd", 14, 8, 64, 6, 9),
    ("s2bd", 14, 64, 64, 2, 0),
)
# regimes the greedy cut cannot produce for a family: {family: {regime: reason}}.  Empty: a search over sides 7 / 14, 8..136 channels,
# batches 1..40 and grids 8..13 found every regime for every family.
IMPOSSIBLE = {}
# The weight-gradient kernels (csrc/conv3x3_wgrad.hip) cut the pixels of a 64 x 64 block into S = max(1, grid / blocks) ranges of K-steps
# (a K-step is 2 rows / 4 rows / 1 image / 2 images of a 56 / 28 / 14 / 7 wide gy map): (stride, side of x, cin, cout, batch, G).
WGRAD_CASES = (
    (1, 7, 64, 64, 1, 8),            # one K-step for eight ranges: seven ranges without a K-step
    (1, 7, 64, 64, 5, 9),            # three K-steps, the last with one image
    (1, 14, 192, 192, 3, 8),         # nine blocks on eight CUs: S == 1
    (1, 14, 64, 128, 5, 9),          # S = 4, five K-steps
    (1, 28, 64, 64, 2, 13),
    (1, 56, 64, 64, 1, 11),
    (2, 14, 64, 64, 3, 9),
    (2, 28, 192, 192, 1, 8),         # S == 1
    (2, 56, 64, 64, 1, 12),
)
FULL_GRID = 256                                                         # the MI355X: what G = 0 means where no device is asked


def wgrad_id(c):
    return "s%d-%dx%d-%d>%d-B%d-G%d" % (c[0], c[1], c[1], c[2], c[3], c[4], c[5])


def case_id(c):
    return "%s-%dx%d-%d>%d-B%d-G%d" % (c[0], c[1], c[1], c[2], c[3], c[4], c[5])


# ---- integer operands of the partition sweep ---------------------------------------------------------------------------------------------
X_MAX, W_MAX, GY_MAX = 16, 4, 16


def int_tensor(shape, bound, gen, device="cpu"):
    """integers of [-bound, bound] as float32: one bf16 piece each"""
    return torch.randint(-bound, bound + 1, shape, generator=gen).float().to(device)


def assert_exact_sum(n_products, a_max, b_max, extra=0):
    """every partial sum of n_products products |a| <= a_max, |b| <= b_max (plus one addend) is an integer float32 holds exactly, so a
    float64 reference rounds to the same float32 whatever the summation order"""
    assert n_products * a_max * b_max + extra < 2 ** 24, (n_products, a_max, b_max, extra)


# ---- the three-piece split, emulated ----------------------------------------------------------------------------------------------------
def bf16_pieces(v):
    """conv_bf16_piece / store_x: v = p0 + p1 + p2, each a bf16 (round to nearest even), residuals in fp32"""
    assert v.dtype == torch.float32
    p0 = v.bfloat16().float()
    r1 = v - p0
    p1 = r1.bfloat16().float()
    p2 = (r1 - p1).bfloat16().float()
    return p0, p1, p2


def split_conv(x, w, drop=(), stride=1):
    """F.conv2d(x, w, None, stride, 1) as the split kernels form it -- the products x_p w_q with p + q <= 2, but those in `drop` -- with
    float64 accumulation.  Returns float64."""
    xp, wp = bf16_pieces(x), bf16_pieces(w)
    out = 0
    for p, q in PRODUCTS:
        if (p, q) not in drop:
            out = out + torch.nn.functional.conv2d(xp[p].double(), wp[q].double(), None, stride, 1)
    return out


def split_wgrad(x, gy, drop=(), stride=1):
    """the weight gradient of the same convolution from the piece products x_p gy_q, float64 accumulation"""
    xp, gp = bf16_pieces(x), bf16_pieces(gy)
    out = 0
    for p, q in PRODUCTS:
        if (p, q) not in drop:
            out = out + torch.nn.grad.conv2d_weight(xp[p].double(), (gy.shape[1], x.shape[1], 3, 3), gp[q].double(), stride, 1)
    return out


# ---- one-product operand patterns (tests/test_gpu_conv_split_exact.py) ------------------------------------------------------------------
def arbitrary_f32(shape, gen):
    """full 24-bit mantissas, exponents 2^-20 .. 2^20, both signs, no zeros"""
    mant = torch.randint(2 ** 23, 2 ** 24, shape, generator=gen).double()
    expo = torch.randint(-20 - 23, 20 - 23 + 1, shape, generator=gen).double()
    sign = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    return (sign * mant * 2.0 ** expo).float()


def sixteen_bit_f32(shape, gen):
    """odd integers below 2^15 with the top bit set, times a power of two: 15 significant bits, so two non-zero bf16 pieces and
    (257 / 256) * w is a float32"""
    mant = (torch.randint(2 ** 13, 2 ** 14, shape, generator=gen) * 2 + 1).double()
    expo = torch.randint(-20, 6, shape, generator=gen).double()
    sign = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    return (sign * mant * 2.0 ** expo).float()


def one_hot_filter(cout, cin):
    """w[co, ci(co), tap(co)] = 1: all nine taps, and input channels in both lane halves (ci % 8 < 4 and >= 4) of several K-steps"""
    w = torch.zeros(cout, cin, 3, 3)
    co = torch.arange(cout)
    ci, tap = (co * 5 + co // 9) % cin, co % 9
    w[co, ci, tap // 3, tap % 3] = 1.0
    assert set(tap.tolist()) == set(range(9)) and {int(c) % 8 < 4 for c in ci} == {True, False}
    return w


HOT_VALUE_11 = 257.0 / 256.0                                             # pieces 1 and 2^-8


def hot_pixels(side):
    """(y, x) of the hot pixel per image, in turn: the corners, borders, the interior"""
    return [(0, 0), (side - 1, side - 1), (0, side - 1), (side - 1, 0), (side // 2, side - 1), (0, side // 2), (side // 2, side // 2), (3, 2)]


def one_hot_maps(batch, channels, side, value=1.0, shift=0):
    """one pixel of one channel per image is `value`: image b has hot_pixels(side)[b + shift], in a channel of its own (both lane halves)"""
    x = torch.zeros(batch, channels, side, side)
    pix = hot_pixels(side)
    chans = [(5 + 11 * (b + shift)) % channels for b in range(batch)]
    assert len(set(chans)) == batch
    for b in range(batch):
        y, xx = pix[(b + shift) % len(pix)]
        x[b, chans[b], y, xx] = value
    return x


def hot_shifts(side, batch):
    """the shifts with which one_hot_maps puts every hot pixel position into some image"""
    return range(0, len(hot_pixels(side)), batch)
