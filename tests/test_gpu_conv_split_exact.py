"""The six piece products of the three-piece bf16 split (conv_split_terms in csrc/conv3x3.hip: x_p w_q with p + q <= 2; the weight
gradient of csrc/conv3x3_wgrad.hip likewise), pinned one by one in EXACT arithmetic.  The 2e-5 bar of tests/test_gpu_conv.py does not
see a split that forms five of them (tests/test_conv_plan_host.py::test_five_products_pass_the_old_bar: 2.4e-6 .. 2.7e-6 of the output
scale), and it is the only bar there for backward-data and the stride-2 backward-data instance (docs/LAB_NOTEBOOK.md section 26).
Here the operands leave exactly one non-zero product x * w per output element: the float64 result is a float32 number, it
owes nothing to the order in which a matrix instruction adds its sixteen products, and the criterion is torch.equal.

  one-hot filter, arbitrary input (24-bit mantissas, exponents 2^-20 .. 2^20): the output is a shifted input channel, bit for bit.
      Needs (0, 0), (1, 0), (2, 0) -- all three pieces of the staged operand -- and the fp32 sum (p2 + p1) + p0.
  one-hot input, arbitrary filter: the output holds filter taps.  Needs (0, 0), (0, 1), (0, 2): pieces 1 and 2 of the filter image,
      which the pack kernels write (sc_conv3x3_pack, sc_conv3x3s2_bd_pack here; the all-filters kernels are compared with them bit
      for bit in tests/test_gpu_conv.py::test_pack_set_equals_single_packs).
  hot input 257/256 (pieces 1 and 2^-8), filter with 15 significant bits: x * w has 24 bits, made exactly by (0, 0), (0, 1), (1, 0) and
      (1, 1).
(p, q) = piece p of the staged map, piece q of the filter; tests/test_conv_plan_host.py shows that leaving out any one of the named
products changes outputs of that pattern.  The hot pixel visits corners, borders and the interior; 72 channels make the K-step count
odd (the PAIRED instance's zero step) and the channel tile ragged; one batch per side puts a tile boundary inside an image."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_plan_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def gen(*seed):
    return torch.Generator().manual_seed(sum(s * 1000 ** i for i, s in enumerate(seed)))


def same(got, ref64, what):
    ref = ref64.float()
    assert torch.equal(ref.double(), ref64), "the reference is not a float32 tensor: " + what
    assert got.shape == ref.shape and torch.equal(got, ref), "%s: %d of %d elements differ, largest difference %g" % (
        what, int((got != ref).sum()), ref.numel(), float((got - ref).abs().max()))
    assert int((ref != 0).sum()) > 0, what


def conv_patterns(n_out, n_red, map_shape, seed):
    """(name, map [batch][n_red][h][w], filter [n_out][n_red][3][3]) of a convolution that reduces over n_red channels"""
    batch, side = map_shape[0], map_shape[2]
    yield "one-hot filter", C.arbitrary_f32(map_shape, gen(1, *seed)), C.one_hot_filter(n_out, n_red)
    for shift in C.hot_shifts(side, batch):
        yield "one-hot input %d" % shift, C.one_hot_maps(batch, n_red, side, 1.0, shift), C.arbitrary_f32((n_out, n_red, 3, 3), gen(2, shift, *seed))
        yield "257/256 input %d" % shift, C.one_hot_maps(batch, n_red, side, C.HOT_VALUE_11, shift), C.sixteen_bit_f32((n_out, n_red, 3, 3), gen(3, shift, *seed))


@pytest.mark.parametrize("side,cin,cout,batch", [(56, 64, 64, 1), (56, 64, 64, 2), (28, 64, 72, 1), (28, 72, 64, 2), (14, 72, 64, 1), (14, 64, 72, 3),
                                                  (7, 64, 72, 2), (7, 72, 64, 6)])
def test_split_forward_and_backward_data_exact(side, cin, cout, batch):
    from shapeclipper_amd import ops
    for name, x, w in conv_patterns(cout, cin, (batch, cin, side, side), (side, cin, batch)):
        x, w = x.to(DEV), w.to(DEV)
        same(ops.conv3x3_forward(x, w, split=True), torch.nn.functional.conv2d(x.double(), w.double(), None, 1, 1), "forward, " + name)
    # backward-data reduces over cout: the filter [cout][cin] is the transpose of a pattern filter [cin][cout]
    for name, gy, wt in conv_patterns(cin, cout, (batch, cout, side, side), (side, cout, batch, 1)):
        gy, w = gy.to(DEV), wt.transpose(0, 1).contiguous().to(DEV)
        same(ops.conv3x3_backward_data(gy, w, split=True), torch.nn.grad.conv2d_input((batch, cin, side, side), w.double(), gy.double(), 1, 1),
             "backward-data, " + name)


@pytest.mark.parametrize("hw,cin,cout,batch", [(56, 64, 64, 1), (56, 64, 72, 2), (28, 72, 64, 1), (28, 64, 64, 3), (14, 64, 72, 2), (14, 72, 64, 6)])
def test_stride2_backward_data_exact(hw, cin, cout, batch):
    """the stride-2 backward-data instance: gy on the hw/2 map, four parity phases, its own filter image (sc_conv3x3s2_bd_pack)"""
    from shapeclipper_amd import ops
    for name, gy, wt in conv_patterns(cin, cout, (batch, cout, hw // 2, hw // 2), (hw, cout, batch, 2)):
        gy, w = gy.to(DEV), wt.transpose(0, 1).contiguous().to(DEV)
        same(ops.conv3x3s2_backward_data(gy, w, hw), torch.nn.grad.conv2d_input((batch, cin, hw, hw), w.double(), gy.double(), 2, 1),
             "stride-2 backward-data, " + name)


@pytest.mark.parametrize("side,cin,cout,batch", [(56, 64, 64, 1), (56, 64, 64, 2), (28, 64, 128, 1), (28, 64, 64, 2), (14, 128, 64, 1), (14, 64, 64, 3),
                                                  (7, 64, 64, 2), (7, 64, 128, 6)])
def test_split_weight_gradient_exact(side, cin, cout, batch):
    """dw[co][ci][tap] = sum over images and pixels of gy x: a hot pixel per image, each in a channel of its own, leaves one product per
    element.  Hot x with arbitrary gy needs (0, 0), (0, 1), (0, 2) of (piece of x, piece of gy); hot gy with arbitrary x the mirror image;
    x = 257/256 with 15-bit gy needs (1, 1)."""
    from shapeclipper_amd import ops
    xs, gs = (batch, cin, side, side), (batch, cout, side, side)
    for shift in C.hot_shifts(side, batch):
        seed = (side, cout, batch, shift)
        for name, x, gy in (("hot x, arbitrary gy", C.one_hot_maps(batch, cin, side, 1.0, shift), C.arbitrary_f32(gs, gen(4, *seed))),
                            ("hot gy, arbitrary x", C.arbitrary_f32(xs, gen(5, *seed)), C.one_hot_maps(batch, cout, side, 1.0, shift)),
                            ("x = 257/256, 15-bit gy", C.one_hot_maps(batch, cin, side, C.HOT_VALUE_11, shift), C.sixteen_bit_f32(gs, gen(6, *seed))),
                            ("gy = 257/256, 15-bit x", C.sixteen_bit_f32(xs, gen(7, *seed)), C.one_hot_maps(batch, cout, side, C.HOT_VALUE_11, shift))):
            x, gy = x.to(DEV), gy.to(DEV)
            same(ops.conv3x3_backward_weight(gy, x, split=True), torch.nn.grad.conv2d_weight(x.double(), (cout, cin, 3, 3), gy.double(), 1, 1),
                 "weight gradient, %s, shift %d" % (name, shift))
