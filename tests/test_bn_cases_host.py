"""Preconditions of the cases of tests/bn_cases.py, checked on the CPU: the float64 restatement is nn.BatchNorm2d's own arithmetic, every
named case has the conditioning it claims, no pre-activation sits on the ReLU kink and no pooling window is tied -- so that
tests/test_gpu_bn_float64.py compares every element rather than "all but the ambiguous ones"."""
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_cases as B  # noqa: E402

ROW_IDS = ["%s-%s-g%d" % (f, "x".join(map(str, s)), g) for f, s, g, _ in B.ROWS]


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _stock64(c):
    """nn.BatchNorm2d(...).double() on the CPU, one call per group in order, + res, ReLU, max-pool."""
    C = c.shape[1]
    bn = nn.BatchNorm2d(C, eps=B.EPS, momentum=B.MOMENTUM, track_running_stats=c.track).double()
    with torch.no_grad():
        bn.weight.copy_(c.gamma)
        bn.bias.copy_(c.beta)
        if c.track:
            bn.running_mean.copy_(c.rm0)
            bn.running_var.copy_(c.rv0)
    bn.train(c.training)
    x = c.x.double().requires_grad_(True)
    res = c.res.double().requires_grad_(True) if c.with_res else None
    y = torch.cat([bn(t) for t in x.chunk(c.groups)], 0)
    if res is not None:
        y = y + res
    if c.relu:
        y = torch.relu(y)
    if c.pool:
        y = F.max_pool2d(y, 3, 2, 1)
    (y * c.cot.double()).sum().backward()
    out = dict(y=y.detach(), dx=x.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad)
    if res is not None:
        out["dres"] = res.grad
    if c.track and c.training:
        out["running_mean"], out["running_var"] = bn.running_mean, bn.running_var
        assert int(bn.num_batches_tracked) == c.groups
    return out


@pytest.mark.parametrize("row", B.ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("training,track", [(True, True), (False, True), (True, False)])
def test_restatement_is_batchnorm2d_in_float64(row, training, track):
    _, shape, groups, pool = row
    c = B.make(shape, groups, relu=True, with_res=not pool, training=training, pool=pool, track=track)
    ref, stock = B.reference(c), _stock64(c)
    for k, v in stock.items():
        assert _rel(ref[k], v) <= 1e-12, (k, _rel(ref[k], v))


def _check_exact(c, what):
    """No exclusion at these inputs: nothing within KINK of the ReLU kink, every pooling window decided by KINK of the scale."""
    ref = B.reference(c)
    scale = float(ref["y"].abs().max())
    if c.relu:
        excluded = int((ref["z"].abs() < B.KINK * scale).sum())
        assert excluded == 0, "%s: %d pre-activations within %.0e of the kink" % (what, excluded, B.KINK)
    if c.pool:
        gap = B.pool_gap(ref["z"])
        C = c.shape[1]
        if c.kind == "flat":                                            # the constant channel: exact ties, decided by scan order
            rows = torch.arange(gap.shape[0]) % C == c.special
            zf = ref["z"][:, c.special]
            assert float(zf.max() - zf.min()) == 0.0 and float(zf.max()) > 0.0
            gap = gap[~rows]
        assert float(gap.min()) >= B.KINK * scale, "%s: pooling gap %.3e of the scale" % (what, float(gap.min()) / scale)


@pytest.mark.parametrize("row", B.ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("training", [True, False])
def test_rows_exclude_nothing(row, training):
    _, shape, groups, pool = row
    for relu, with_res in ([(True, False)] if pool else [(True, False), (True, True)]):
        c = B.make(shape, groups, relu=relu, with_res=with_res, training=training, pool=pool)
        _check_exact(c, "%s g%d" % (shape, groups))
        k, d = B.conditioning(c.x, groups)
        if c.x[0, 0].numel() * (shape[0] // groups) >= 3:               # the bulk regime: kappa 0.3, delta 1
            assert abs(k - 0.3) <= 0.03 and abs(d - 1.0) <= 0.1, (k, d)


COND_CASES = [(n, kind, k, d, shape, pool) for n, kind, k, d in B.COND for shape, pool in B.COND_SHAPES] + \
             [("first_pixel_64", "first_pixel", 0.3, 64.0, shape, pool) for shape, pool in B.FIRST_PIXEL_64]


@pytest.mark.parametrize("name,kind,kappa,delta,shape,pool", COND_CASES, ids=["%s-%s" % (c[0], "x".join(map(str, c[4]))) for c in COND_CASES])
def test_conditioning_cases_are_what_they_claim(name, kind, kappa, delta, shape, pool):
    c = B.make(shape, 1, kind=kind, kappa=kappa, delta=delta, pool=pool)
    _check_exact(c, name)
    special = (c.special,) if kind in ("flat", "tiny_var") else ()
    k, d = B.conditioning(c.x, 1, skip=special)
    print("%s %s: kappa %.4g (claimed %g), delta %.4g (claimed %g)" % (name, shape, k, kappa, d, delta))
    assert abs(k - kappa) <= 0.1 * kappa and abs(d - delta) <= 0.1 * delta
    ch = c.x[:, c.special].double()
    if kind == "flat":
        assert float(ch.max() - ch.min()) == 0.0
        ref = B.reference(c)
        assert float(ref["save_rstd"][0, c.special]) == pytest.approx(B.EPS ** -0.5, rel=1e-12)
    if kind == "tiny_var":
        ks, ds = B.conditioning(c.x[:, c.special:c.special + 1], 1)
        print("    channel %d alone: kappa %.4g, delta %.4g" % (c.special, ks, ds))
        assert abs(ks - 1e4) <= 1e3 and abs(ds - 1.0) <= 0.1


def test_delta_64_does_not_exist_at_the_small_shapes():
    """|x_first - mu| / sigma <= sqrt(n - 1) for n values: 15.97, 39.6, 22.6 at the three conditioning shapes."""
    for (shape, _), (big, _) in zip(B.COND_SHAPES, B.FIRST_PIXEL_64):
        n, nb = shape[0] * shape[2] * shape[3], big[0] * big[2] * big[3]
        assert (n - 1) ** 0.5 < 64 < (nb - 1) ** 0.5
        assert B.fused_takes(shape[0], shape[1], shape[2] * shape[3], 1) == B.fused_takes(big[0], big[1], big[2] * big[3], 1)
        assert (shape[3] & 1) == (big[3] & 1) and ((shape[2] * shape[3]) & 3 == 0) == ((big[2] * big[3]) & 3 == 0)


def test_rows_reach_the_launch_form_they_name():
    for form, (N, C, H, W), G, pool in B.ROWS:
        assert N % G == 0
        fused = not pool and B.fused_takes(N, C, H * W, G)
        assert fused == (form.startswith("one_launch") and (N, G) not in ((105, 1), (105, 3))), (form, N, C, H, W, G)
        if form == "one_launch_float4" or form == "two_launch_float4":
            assert (H * W) & 3 == 0
        if form.endswith("scalar"):
            assert (H * W) & 3
        if form.startswith("stem"):
            assert (W & 1) == (form == "stem_odd")
    assert B.bn_splits(8, 8, 1) == 8 and B.bn_splits(32, 32, 2) == 32 and B.bn_splits(2, 300, 5) == 2
    for a, b in B.BOUNDARY_PAIRS:
        va, vb = [s[0] * (s[2] * s[3] if (s[2] * s[3]) & 3 else s[2] * s[3] // 4) for s in (a, b)]
        assert (va, vb) == (5096, 5145)


def test_partial_sum_workspace_holds_every_shape():
    """ops._bn_partial promises at most 2 * (2048 + C * G) floats: C * G * S pairs are written."""
    try:
        from shapeclipper_amd import _lib
        splits = _lib.load().sc_bn_splits
    except Exception:       # noqa: BLE001 -- no library on this machine: the restated rule alone
        splits = None
    shapes = [(s, g) for _, s, g, _ in B.ROWS] + [(s, 1) for s, _ in B.COND_SHAPES + B.FIRST_PIXEL_64] + [(s, 3) for s, _ in B.SEQ_SHAPES]
    for (N, C, H, W), G in shapes:
        S = B.bn_splits(N // G, C, G)
        if splits is not None and G == 1:
            assert int(splits(N, C)) == S
        assert C * G * S * 2 <= 2 * (2048 + C * G), ((N, C, H, W), G, S)
