"""Fused BatchNorm (+ residual add, ReLU, stem max-pool) kernels of csrc/bn_act.hip against the stock torch operators
they replace inside the ResNet encoders (torchvision BasicBlock / stem semantics).
Tolerance: fp32, 2e-5 of the tensor's scale for outputs and input gradients (different summation order only).
The bars against float64 (every launch form, ill-conditioned channels, chains of running-statistics updates): tests/test_gpu_bn_float64.py."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _close(a, b, tol=2e-5, what="", where=None):
    scale = max(float(b.abs().max()), 1e-6)
    diff = (a - b).abs()
    if where is not None:
        diff = diff * where
    err = float(diff.max())
    assert err <= tol * scale + 1e-7, "%s: max err %.3e (scale %.3e)" % (what, err, scale)


def _stock(bn, x, res, relu):
    out = bn(x)
    if res is not None:
        out = out + res
    return torch.relu(out) if relu else out


# (32, 512, 7, 7) and (8, 256, 14, 14): the one-launch form for many-channel small maps (scalar and float4 variants);
# (32, 512, 1, 1) and (6, 70, 1, 1): the 1 x 1 maps of the heads' BatchNorms (one-launch form / two-launch form)
@pytest.mark.parametrize("shape", [(8, 64, 56, 56), (4, 16, 7, 7), (3, 5, 6, 10), (32, 512, 7, 7), (8, 256, 14, 14), (32, 512, 1, 1), (6, 70, 1, 1),
                                   (1, 8, 4, 4)])
@pytest.mark.parametrize("relu,with_res", [(True, False), (True, True), (False, False), (False, True)])
@pytest.mark.parametrize("training", [True, False])
def test_bn_act_matches_torch(shape, relu, with_res, training):
    from shapeclipper_amd.functional import bn_act
    torch.manual_seed(0)
    N, C, H, W = shape
    dev = "cuda"
    x0 = (torch.randn(shape, device=dev) * 1.7 + 0.4)
    r0 = torch.randn(shape, device=dev) if with_res else None
    cot = torch.randn(shape, device=dev)
    bn_a = nn.BatchNorm2d(C).to(dev)
    with torch.no_grad():
        bn_a.weight.copy_(torch.randn(C) * 0.5 + 1.0)       # includes negative scales
        bn_a.bias.copy_(torch.randn(C) * 0.3)
        bn_a.running_mean.copy_(torch.randn(C) * 0.2)
        bn_a.running_var.copy_(torch.rand(C) + 0.5)
    bn_a.train(training)
    if relu:
        # keep every pre-activation away from the ReLU kink: an element within rounding of 0 may legitimately land on
        # either side of it in two fp32 implementations, which would flip its gradient (and move dgamma/dbeta)
        probe = copy.deepcopy(bn_a)
        for _ in range(4):
            with torch.no_grad():
                z = probe(x0) + (r0 if with_res else 0)
                near = z.abs() < 1e-3
                if not bool(near.any()):
                    break
                x0[near] += 0.25
    bn_b = copy.deepcopy(bn_a)
    bn_b.train(training)
    outs = []
    for bn, fn in ((bn_a, _stock), (bn_b, lambda bn, x, r, relu: bn_act(bn, x, residual=r, relu=relu))):
        x = x0.clone().requires_grad_(True)
        r = r0.clone().requires_grad_(True) if with_res else None
        y = fn(bn, x, r, relu)
        (y * cot).sum().backward()
        outs.append((y.detach(), x.grad, r.grad if with_res else None, bn.weight.grad, bn.bias.grad,
                     bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)))
    ref, got = outs
    _close(got[0], ref[0], what="y")
    # an output within rounding of the ReLU kink may land on either side of it: such elements (a handful per million)
    # are left out of the element-wise gradient comparison
    away = (ref[0].abs() > 1e-5).float() if relu else None
    _close(got[1], ref[1], tol=5e-5, what="dx", where=away)
    if with_res:
        _close(got[2], ref[2], what="dres", where=away)
    _close(got[3], ref[3], tol=1e-4, what="dgamma")
    _close(got[4], ref[4], tol=1e-4, what="dbeta")
    _close(got[5], ref[5], what="running_mean")
    _close(got[6], ref[6], what="running_var")
    assert got[7] == ref[7]


@pytest.mark.parametrize("shape", [(4, 8, 30, 30), (2, 4, 17, 23), (8, 64, 112, 112)])
@pytest.mark.parametrize("training", [True, False])
def test_bn_relu_maxpool_matches_torch(shape, training):
    from shapeclipper_amd.functional import bn_relu_maxpool
    torch.manual_seed(1)
    N, C, H, W = shape
    dev = "cuda"
    x0 = torch.randn(shape, device=dev) * 1.3 - 0.2
    bn_a = nn.BatchNorm2d(C).to(dev)
    with torch.no_grad():
        bn_a.weight.copy_(torch.randn(C) * 0.5 + 1.0)
        bn_a.bias.copy_(torch.randn(C) * 0.3)
    bn_b = copy.deepcopy(bn_a)
    bn_a.train(training)
    bn_b.train(training)
    xa = x0.clone().requires_grad_(True)
    ya = F.max_pool2d(torch.relu(bn_a(xa)), 3, 2, 1)
    cot = torch.randn_like(ya)
    (ya * cot).sum().backward()
    xb = x0.clone().requires_grad_(True)
    yb = bn_relu_maxpool(bn_b, xb)
    assert yb.shape == ya.shape
    (yb * cot).sum().backward()
    _close(yb.detach(), ya.detach(), what="y")
    _close(xb.grad, xa.grad, tol=5e-5, what="dx")
    _close(bn_b.weight.grad, bn_a.weight.grad, tol=1e-4, what="dgamma")
    _close(bn_b.bias.grad, bn_a.bias.grad, tol=1e-4, what="dbeta")
    _close(bn_b.running_mean, bn_a.running_mean, what="running_mean")
    _close(bn_b.running_var, bn_a.running_var, what="running_var")
    assert int(bn_b.num_batches_tracked) == int(bn_a.num_batches_tracked)


def test_resnet18_fused_equals_stock_operators():
    from shapeclipper_amd.model import resnet
    torch.manual_seed(2)
    net = resnet.build("resnet18").cuda().train()
    x = torch.randn(4, 3, 224, 224, device="cuda")
    res = []
    for fused in (False, True):
        resnet.FUSED_BN = fused
        try:
            m = copy.deepcopy(net)
            y = m(x)
            y.square().mean().backward()
            res.append((y.detach(), m.conv1.weight.grad.clone(), m.layer4[1].bn2.weight.grad.clone(),
                        m.layer1[0].bn1.running_var.clone()))
        finally:
            resnet.FUSED_BN = True
    # 17 BN layers deep: rounding differences (and the odd ReLU-kink flip) are amplified -> relative L2 error
    for a, b, name in zip(res[1], res[0], ("logits", "d conv1.weight", "d layer4.1.bn2.weight", "running_var")):
        rel = float((a - b).norm() / b.norm().clamp_min(1e-12))
        assert rel < 5e-3, "%s: relative L2 error %.3e" % (name, rel)


@pytest.mark.parametrize("shape,groups", [((6, 16, 14, 14), 3), ((8, 64, 28, 28), 2), ((96, 512, 1, 1), 3), ((12, 256, 14, 14), 3), ((8, 512, 7, 7), 4), ((128, 96, 1, 1), 4), ((4, 8, 5, 7), 4)])
@pytest.mark.parametrize("with_res", [False, True])
def test_grouped_bn_equals_consecutive_calls(shape, groups, with_res):
    """groups = G: the result (outputs, gradients, running statistics, num_batches_tracked) of G consecutive
    nn.BatchNorm2d calls on the G sub-batches -- what the reference does when it runs the same network on the input
    view, the neighbour view and the mirrored image one after the other."""
    from shapeclipper_amd.functional import bn_act
    torch.manual_seed(3)
    N, C, H, W = shape
    x0 = torch.randn(shape, device="cuda") * torch.linspace(0.5, 2.0, N, device="cuda").view(N, 1, 1, 1) + 0.3
    r0 = torch.randn(shape, device="cuda") if with_res else None
    bn_a = nn.BatchNorm2d(C).cuda().train()
    with torch.no_grad():
        bn_a.weight.copy_(torch.rand(C) + 0.5)
        bn_a.bias.copy_(torch.randn(C) * 0.3)
        probe = copy.deepcopy(bn_a)
        for _ in range(4):
            z = torch.cat([probe(c) for c in x0.chunk(groups)], 0) + (r0 if with_res else 0)
            near = z.abs() < 1e-3
            if not bool(near.any()):
                break
            x0[near] += 0.25
    bn_b = copy.deepcopy(bn_a)
    cot = torch.randn(shape, device="cuda")
    xa = x0.clone().requires_grad_(True)
    ra = r0.clone().requires_grad_(True) if with_res else None
    ya = torch.cat([bn_a(c) for c in xa.chunk(groups)], 0)
    ya = torch.relu(ya + ra if with_res else ya)
    (ya * cot).sum().backward()
    xb = x0.clone().requires_grad_(True)
    rb = r0.clone().requires_grad_(True) if with_res else None
    yb = bn_act(bn_b, xb, residual=rb, relu=True, groups=groups)
    (yb * cot).sum().backward()
    _close(yb.detach(), ya.detach(), what="y")
    _close(xb.grad, xa.grad, tol=5e-5, what="dx")
    if with_res:
        _close(rb.grad, ra.grad, what="dres")
    _close(bn_b.weight.grad, bn_a.weight.grad, tol=1e-4, what="dgamma")
    _close(bn_b.bias.grad, bn_a.bias.grad, tol=1e-4, what="dbeta")
    _close(bn_b.running_mean, bn_a.running_mean, what="running_mean")
    _close(bn_b.running_var, bn_a.running_var, what="running_var")
    assert int(bn_b.num_batches_tracked) == int(bn_a.num_batches_tracked) == groups


def test_resnet18_grouped_pass_equals_separate_passes():
    from shapeclipper_amd.model import resnet
    torch.manual_seed(4)
    net = resnet.build("resnet18").cuda().train()
    xs = [torch.randn(3, 3, 224, 224, device="cuda") * s for s in (1.0, 0.5, 2.0)]
    a, b = copy.deepcopy(net), copy.deepcopy(net)
    ya = torch.cat([a(x) for x in xs], 0)
    yb = b(torch.cat(xs, 0), groups=3)
    w = torch.randn_like(ya)
    (ya * w).sum().backward()
    (yb * w).sum().backward()
    rel = lambda u, v: float((u - v).norm() / v.norm().clamp_min(1e-12))
    assert rel(yb.detach(), ya.detach()) < 2e-3
    # 3 images per BN group, 17 BN layers on the way back: fp32 summation-order differences between a 9-image and three 3-image
    # convolution launches are amplified to a few 1e-3 (observed 2e-3 .. 5.4e-3 depending on the convolution kernels' K split)
    assert rel(b.conv1.weight.grad, a.conv1.weight.grad) < 1.5e-2
    assert rel(b.layer3[0].bn1.running_var, a.layer3[0].bn1.running_var) < 1e-4
    assert int(b.bn1.num_batches_tracked) == int(a.bn1.num_batches_tracked) == 3
