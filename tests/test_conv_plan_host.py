"""The work partition of the 3x3 convolution launches (conv_plan / conv_span_cut in csrc/conv3x3.hip, exported as sc_conv3x3_plan) and
the operand patterns of the exact split tests, on the host: no GPU.  Every plan is asked with a positive grid, so nothing here asks a
device.  Checked: over a sweep of families, grids, K-step counts, tile counts and both span modes, a Python replay of conv3x3_kernel's
items and of conv3x3_fixup_kernel's reads (tests/conv_plan_cases.py) counts every K-step of every tile exactly once; the exported span
table is the greedy cut restated in Python; the GPU case list of tests/test_gpu_conv_plan.py contains every regime for every family;
and, for the exact tests of the six piece products (tests/test_gpu_conv_split_exact.py), that each operand pattern loses its exactness
when any one of the products it is meant to pin is left out -- while on random operands no single missing product shows at the 2e-5 bar
of tests/test_gpu_conv.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_plan_cases as C  # noqa: E402

GRIDS = tuple(range(8, 41)) + (63, 64, 65, 127, 128, 200, 224, 240, 248, 255, 256)
NKS = (1, 2, 3, 4, 8, 9, 16, 32, 64)
INVALID = 1                       # hipErrorInvalidValue


def tile_targets(G):
    edge = {1, 2, G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1, 3 * G + 1}
    return sorted(t for t in edge | set(range(3, 3 * G, max(1, (3 * G) // 7))) if t >= 1)


def shape_for(family, tiles, nk):
    """(side, batch, cin, cout) whose plan has `tiles` tiles (stride-2 backward-data: the multiple of 4 next to it) of nk K-steps (split:
    the even number next to it): 49-pixel maps, one channel tile"""
    side = 7 if family in ("fp32", "split") else 14
    pt = {"fp32": 128, "split": 256, "s2fwd": 256, "s2bd": 256}[family]
    ptiles = max(1, (tiles + 2) // 4) if family == "s2bd" else tiles
    batch = (pt * (ptiles - 1) + 1 + 48) // 49
    cin, cout = (64, 8 * nk) if family == "s2bd" else (8 * nk, 64)
    return side, batch, cin, cout, ptiles * (4 if family == "s2bd" else 1)


@pytest.mark.parametrize("equal", [False, True], ids=["table", "equal"])
@pytest.mark.parametrize("family", C.FAMILIES)
def test_replay_counts_every_k_step_once(family, equal):
    """C.replay asserts: gperm is a permutation; spans are at most nk long and touch at most two tiles; every tile of the whole rounds is
    stored once; for every shared tile the partials the fix-up reads exist, were written by the workgroup it names, abut in K order and
    cover [0, nk); a tile stored whole is never also summed; no partial is left unread.  With the table, it is the greedy cut."""
    n = 0
    seen = set()
    for G in GRIDS:
        for nk in NKS:
            for target in tile_targets(G):
                side, batch, cin, cout, tiles = shape_for(family, target, nk)
                p = C.plan(family, side, batch, cin, cout, G, equal)
                assert isinstance(p, dict), (p, family, side, batch, cin, cout, G)
                assert (p["tiles"], p["nk"]) == C.expected_head(family, side, batch, cin, cout, p) and p["tiles"] == tiles and p["G"] == G
                assert p["nk"] == (nk + 1 & ~1 if family == "split" else nk)
                assert p["table"] == (0 if equal or p["tail_tiles"] == 0 else 1)
                C.replay(p)
                if p["table"]:
                    assert p["spans"] == C.greedy_cut(p["tail_tiles"], p["nk"], G, p["ov2"]), (family, side, batch, cin, cout, G)
                    assert p["ov2"] == (2 if p["PT"] >= 512 else 3)
                seen.add((p["rounds"] > 0, p["tail_tiles"] > 0, p["rounds"] > 1))
                n += 1
    assert len(seen) >= 5 and n > 3000        # no tail / tail only / both, one and several rounds


def test_plan_geometry_of_every_instance():
    """PT and CT per family and map side (the tile shapes of csrc/conv3x3.hip), and the head of the plan from the shapes"""
    want = {("fp32", 56): (512, 64), ("fp32", 28): (256, 128), ("fp32", 14): (256, 128), ("fp32", 7): (128, 128),
            ("split", 56): (512, 64), ("split", 28): (512, 64), ("split", 14): (512, 64), ("split", 7): (256, 64),
            ("s2fwd", 56): (256, 64), ("s2fwd", 28): (256, 64), ("s2fwd", 14): (256, 64),
            ("s2bd", 56): (512, 64), ("s2bd", 28): (512, 64), ("s2bd", 14): (256, 64)}
    for (family, side), (pt, ct) in want.items():
        for batch, cin, cout in ((1, 64, 64), (3, 72, 136), (5, 128, 64)):
            p = C.plan(family, side, batch, cin, cout, 256)
            assert (p["PT"], p["CT"]) == (pt, ct), (family, side)
            assert (p["tiles"], p["nk"]) == C.expected_head(family, side, batch, cin, cout, p)
            C.replay(p)


def test_plan_refuses_what_the_launch_refuses():
    assert C.plan("fp32", 14, 1, 20, 64, 256) == INVALID and C.plan("fp32", 14, 0, 64, 64, 256) == INVALID
    assert C.plan("s2bd", 14, 1, 64, 20, 256) == INVALID                 # the reduction channels are the forward's cout
    assert isinstance(C.plan("s2bd", 14, 1, 20, 64, 256), dict)
    assert C.plan("fp32", 15, 1, 64, 64, 256) == -1 and C.plan("s2fwd", 7, 1, 64, 64, 256) == -1 and C.plan("s2bd", 7, 1, 64, 64, 256) == -1
    from shapeclipper_amd import _lib
    lib = _lib.load()
    assert lib.sc_conv3x3_plan(4, 14, 1, 64, 64, 256, 0, (C.ctypes.c_int * 10)(), None) == -1
    assert lib.sc_conv3x3_plan(0, 14, 1, 64, 64, 256, 0, None, None) == INVALID
    assert "sc_conv3x3_plan" in _lib.TIMING_SKIP


def _case_plan(c):
    family, side, cin, cout, batch, G = c
    return C.plan(family, side, batch, cin, cout, G or C.FULL_GRID)


@pytest.mark.parametrize("case", C.GPU_CASES, ids=C.case_id)
def test_gpu_case_replays(case):
    family, side, cin, cout, batch, G = case
    assert side <= 14 and batch <= 40 and max(cin, cout) <= 512, "the sweep keeps to small maps"
    C.replay(_case_plan(case))


@pytest.mark.parametrize("family", C.FAMILIES)
def test_gpu_cases_contain_every_regime(family):
    """Every regime of the partition is run against float64 by some row of the GPU case list, for every family (a regime the cut cannot
    produce for a family is named in C.IMPOSSIBLE with its reason), and one row per family runs on the full grid."""
    rows = [c for c in C.GPU_CASES if c[0] == family]
    got = {c: C.regimes(c[0], c[1], c[4], c[2], c[3], _case_plan(c)) for c in rows}
    for c in rows:
        print("%-28s %s" % (C.case_id(c), " ".join(sorted(got[c]))))
    impossible = C.IMPOSSIBLE.get(family, {})
    assert all(r in C.REGIMES and reason for r, reason in impossible.items())
    missing = set(C.REGIMES) - set().union(*got.values()) - set(impossible)
    assert not missing, (family, sorted(missing))
    assert not set(impossible) & set().union(*got.values()), "a regime listed as impossible occurs"
    assert any(c[5] == 0 for c in rows), "one case per family stays on the full grid"
    assert all(c[5] == 0 or 8 <= c[5] < C.FULL_GRID for c in rows)


# ---- the operand patterns of tests/test_gpu_conv_split_exact.py ---------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_split_premises():
    """The three pieces add up to the value; the fp32 order (p2 + p1) + p0 returns it; most values have a third piece; the products of
    the 257/256 pattern are float32 numbers the four piece products make exactly, and (1, 1) matters for most of them."""
    v = C.arbitrary_f32((1 << 20,), _gen(1))
    assert (v != 0).all() and (v.abs() >= 2.0 ** -20).all() and (v.abs() < 2.0 ** 21).all()
    p0, p1, p2 = C.bf16_pieces(v)
    assert torch.equal(p0.double() + p1.double() + p2.double(), v.double())
    assert torch.equal((p2 + p1) + p0, v)
    assert float((p2 != 0).float().mean()) > 0.9
    w = C.sixteen_bit_f32((1 << 20,), _gen(2))
    x = torch.full_like(w, C.HOT_VALUE_11)
    assert torch.equal((x.double() * w.double()).float().double(), x.double() * w.double())
    xp, wp = C.bf16_pieces(x), C.bf16_pieces(w)
    assert (xp[0] == 1).all() and (xp[1] == 2.0 ** -8).all() and (xp[2] == 0).all() and (wp[2] == 0).all()
    four = sum(xp[p].double() * wp[q].double() for p, q in ((0, 0), (0, 1), (1, 0), (1, 1)))
    assert torch.equal(four, x.double() * w.double())
    assert float((wp[1] != 0).float().mean()) > 0.9                      # leaving out (1, 1) changes these outputs


def _patterns(cin=16, cout=24, side=7, batch=3):
    """name -> (x, w, the products the pattern pins)"""
    return {"one-hot filter": (C.arbitrary_f32((batch, cin, side, side), _gen(3)), C.one_hot_filter(cout, cin), ((0, 0), (1, 0), (2, 0))),
            "one-hot input": (C.one_hot_maps(batch, cin, side), C.arbitrary_f32((cout, cin, 3, 3), _gen(4)), ((0, 0), (0, 1), (0, 2))),
            "257/256 input": (C.one_hot_maps(batch, cin, side, C.HOT_VALUE_11), C.sixteen_bit_f32((cout, cin, 3, 3), _gen(5)),
                              ((0, 0), (0, 1), (1, 0), (1, 1)))}


@pytest.mark.parametrize("name", ["one-hot filter", "one-hot input", "257/256 input"])
def test_pattern_pins_its_products(name):
    """With all six products the emulated split gives the float64 convolution exactly, which is a float32 tensor (one non-zero product
    per output element); without any one of the pinned products at least one output changes."""
    x, w, pinned = _patterns()[name]
    y64 = torch.nn.functional.conv2d(x.double(), w.double(), None, 1, 1)
    assert torch.equal(y64.float().double(), y64) and torch.equal(C.split_conv(x, w), y64)
    for prod in pinned:
        wrong = C.split_conv(x, w, drop=(prod,)).float() != y64.float()
        print("%s without product %r: %d of %d outputs change" % (name, prod, int(wrong.sum()), wrong.numel()))
        assert wrong.any(), prod
    # the same operands as a weight gradient: x with a one-hot / arbitrary gy of the output's shape
    gy = {"one-hot filter": C.one_hot_maps(x.shape[0], w.shape[0], x.shape[2]), "one-hot input": C.arbitrary_f32(y64.shape, _gen(6)),
          "257/256 input": C.sixteen_bit_f32(y64.shape, _gen(7))}[name]
    d64 = torch.nn.grad.conv2d_weight(x.double(), w.shape, gy.double(), 1, 1)
    assert torch.equal(d64.float().double(), d64) and torch.equal(C.split_wgrad(x, gy), d64)
    for prod in pinned:
        assert (C.split_wgrad(x, gy, drop=(prod,)).float() != d64.float()).any(), prod


def test_five_products_pass_the_old_bar():
    """Why 2e-5 of the output scale (tests/test_gpu_conv.py) does not pin the six products: on that file's random operands (14 x 14,
    64 > 64) a split that leaves out any ONE product stays eight times below the bar.  That bar is all that file asks of backward-data
    and of the stride-2 backward-data instance.  (Its second bar, e_split < 2 e_fp32 + 2e-7, is asked of the stride-1 forward pass
    only; the fp32 kernel measures 2e-7 .. 5e-7 there, not the 3e-6 of that file's header, so a five-product FORWARD pass does fail it
    -- measured with a library built without one product: 2.2e-6 .. 3.4e-6 against bars of 6e-7 .. 1.2e-6.)"""
    g = _gen(14 + 64 + 2)
    x = torch.randn(2, 64, 14, 14, generator=g) * torch.rand(2, 64, 1, 1, generator=g) * 4
    w = torch.randn(64, 64, 3, 3, generator=g) * (2.0 / (9 * 64)) ** 0.5
    y64 = torch.nn.functional.conv2d(x.double(), w.double(), None, 1, 1)
    rel = lambda y: float((y - y64).abs().max() / y64.abs().max())
    e_all = rel(C.split_conv(x, w))
    print("all six products: %.1e of max" % e_all)
    assert e_all < 1e-7
    for prod in ((0, 2), (2, 0), (1, 1)):
        e = rel(C.split_conv(x, w, drop=(prod,)))
        print("without %r: %.1e of max" % (prod, e))
        assert 20 * e_all < e < 2e-5 / 4
