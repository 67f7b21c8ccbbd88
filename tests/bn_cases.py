"""Seeded inputs and the float64 reference of the BatchNorm kernels of csrc/bn_act.hip.  Plain module, no GPU: tests/test_bn_cases_host.py
checks the cases' preconditions on the CPU, tests/test_gpu_bn_float64.py compares the kernels (and torch's own fp32 BatchNorm) with the
reference.

Reference: `forward64` restates relu(batch_norm(x) [+ res]) and the stem's maxpool3x3/2/1(relu(bn(x))) per channel and group with a
two-pass mean and variance (biased for the normalisation, unbiased with momentum for the running statistics, `groups` updates in group
order); gradients come from float64 autograd through it.  Inputs are drawn in fp32 and promoted, so the reference sees the numbers the
kernel sees.

Conditioning of a case, over all channels and groups, in float64:
    kappa = max |mu| / sigma                       (how far the channel sits from zero, in standard deviations)
    delta = max |x_first - mu| / sigma             (x_first = x[n0, c, 0, 0]: the element the kernels take as their variance shift)
Every (channel, group) block is standardised exactly, so a case has the kappa and delta it names.  delta <= sqrt(n - 1) for n values, so
delta = 64 does not exist at the shapes of the other conditioning cases (n = 256, 1568, 512): it runs at the smallest shapes that reach
the same kernels and hold it (n >= 5120, FIRST_PIXEL_64).

What makes the comparison exact (asserted on the CPU): every pre-activation is at least 1e-3 of the output scale away from the ReLU kink,
and the winner of every pooling window beats the runner-up by at least 1e-3 of the scale (inputs are nudged in float64 until they do).
A channel that is constant (`flat`) ties every window exactly, in every precision: the first element in scan order wins in all of them."""
from functools import lru_cache

import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64
EPS, MOMENTUM = 1e-5, 0.1
KINK = 1e-3                  # of the output scale: the asserted distance; the generator leaves twice that
SPECIAL = 3                  # the channel that `flat` / `tiny_var` replace
NEG, ZERO = 1, 2             # channels with a negative / a zero gamma (no zero gamma in the stem: it would tie every pooling window)

# (form, shape, groups, pool)
ROWS = [
    ("two_launch_float4", (4, 16, 8, 8), 1, False), ("two_launch_float4", (4, 16, 8, 8), 2, False),
    ("two_launch_float4", (10, 300, 4, 4), 5, False),                   # C >= 256 but G > 4 (N must be a multiple of G: 10, not 6)
    ("two_launch_float4", (3, 5, 6, 10), 1, False), ("two_launch_float4", (3, 5, 6, 10), 3, False),        # HW = 60: still float4
    ("two_launch_scalar", (3, 5, 7, 9), 1, False), ("two_launch_scalar", (3, 5, 7, 9), 3, False),          # HW = 63
    ("two_launch_scalar", (6, 70, 1, 1), 2, False),
    ("two_launch_split", (8, 8, 14, 14), 1, False),                     # S = 8 = Ng
    ("two_launch_split", (64, 32, 4, 4), 2, False),                     # S = 32
    ("one_launch_float4", (104, 256, 14, 14), 1, False),                # 5096 vectors: one launch
    ("one_launch_float4", (105, 256, 14, 14), 1, False),                # 5145: two launches
    ("one_launch_scalar", (104, 256, 7, 7), 1, False),                  # 5096
    ("one_launch_scalar", (105, 256, 7, 7), 1, False), ("one_launch_scalar", (105, 256, 7, 7), 3, False),
    ("one_launch_groups", (8, 256, 14, 14), 4, False), ("one_launch_groups", (12, 256, 7, 7), 3, False),
    ("one_launch_groups", (96, 512, 1, 1), 3, False),
    ("stem_even", (2, 4, 16, 16), 1, True), ("stem_even", (2, 4, 16, 16), 2, True),
    ("stem_even", (3, 4, 10, 6), 1, True),                              # Ho = 5: not a multiple of the strip height
    ("stem_odd", (2, 4, 17, 23), 1, True), ("stem_odd", (2, 4, 17, 23), 2, True), ("stem_odd", (4, 3, 5, 7), 2, True),
]
BOUNDARY_PAIRS = [((104, 256, 14, 14), (105, 256, 14, 14)), ((104, 256, 7, 7), (105, 256, 7, 7))]

# conditioning cases: (name, kind, kappa, delta); applied to COND_SHAPES
COND = [("bulk", "bulk", 0.3, 1.0), ("offset_10", "offset", 10.0, 1.0), ("offset_100", "offset", 100.0, 1.0),
        ("offset_1000", "offset", 1000.0, 1.0), ("first_pixel_8", "first_pixel", 0.3, 8.0), ("flat", "flat", 0.3, 1.0),
        ("tiny_var", "tiny_var", 0.3, 1.0)]
COND_SHAPES = [((4, 16, 8, 8), False), ((8, 256, 14, 14), False), ((2, 4, 16, 16), True)]
FIRST_PIXEL_64 = [((20, 16, 16, 16), False), ((80, 256, 8, 8), False), ((2, 4, 52, 52), True)]      # n = 5120, 5120, 5408 per channel
SEQ_SHAPES = [((6, 16, 8, 8), False), ((12, 256, 7, 7), False), ((6, 4, 16, 16), True)]             # groups = 3



class Case:
    """One seeded input set (hashed by identity: `make` returns the same object for the same arguments)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def bn_splits(Ng, C, G):
    """Blocks per (channel, group) of the two-launch form (csrc/bn_act.hip, bn_splits)."""
    S = (2048 + C * G - 1) // (C * G)
    return max(1, min(S, Ng, 32))


def fused_takes(N, C, HW, G):
    vecs = N * HW if HW & 3 else N * (HW >> 2)
    return C >= 256 and G <= 4 and vecs <= 512 * 10


def forward64(x, res, gamma, beta, rm, rv, training, groups, relu, pool, momentum=MOMENTUM, eps=EPS):
    """-> y, z (pre-activation), save_mean [G,C], save_rstd [G,C], running_mean, running_var (new tensors; rm / rv may be None)."""
    N, C = x.shape[:2]
    Ng = N // groups
    zs, means, rstds = [], [], []
    for g in range(groups):
        xg = x[g * Ng:(g + 1) * Ng]
        if training:
            n = xg.numel() // C
            mean = xg.mean((0, 2, 3))
            var = (xg - mean.view(1, C, 1, 1)).square().mean((0, 2, 3))
            if rm is not None:
                rm = (1 - momentum) * rm + momentum * mean.detach()
                rv = (1 - momentum) * rv + momentum * var.detach() * (n / (n - 1))
        else:
            mean, var = rm, rv
        rstd = (var + eps).rsqrt()
        zs.append((xg - mean.view(1, C, 1, 1)) * (rstd * gamma).view(1, C, 1, 1) + beta.view(1, C, 1, 1))
        means.append(mean.detach())
        rstds.append(rstd.detach())
    z = torch.cat(zs, 0)
    if res is not None:
        z = z + res
    y = torch.relu(z) if relu else z
    if pool:
        y = F.max_pool2d(y, 3, 2, 1)
    return y, z, torch.stack(means), torch.stack(rstds), rm, rv


def _blocks(x, groups):
    """[N,C,H,W] -> [G,C,n]: the values of every (group, channel) in the kernels' order (element 0 = x[n0, c, 0, 0])."""
    N, C, H, W = x.shape
    return x.view(groups, N // groups, C, H * W).permute(0, 2, 1, 3).reshape(groups, C, -1)


def _unblocks(b, shape, groups):
    N, C, H, W = shape
    return b.view(groups, C, N // groups, H * W).permute(0, 2, 1, 3).reshape(shape).contiguous()


def conditioning(x, groups, skip=()):
    """(kappa, delta) in float64; channels in `skip` (a constant channel has no sigma) are left out."""
    b = _blocks(x.double(), groups)
    mu = b.mean(-1)
    sd = (b - mu[..., None]).square().mean(-1).sqrt()
    keep = [c for c in range(x.shape[1]) if c not in skip]
    k = (mu.abs() / sd)[:, keep]
    d = ((b[..., 0] - mu).abs() / sd)[:, keep]
    return float(k.max()), float(d.max())


def _standardised(g, G, C, n, delta):
    """[G,C,n] float64: mean 0, variance 1 exactly, element 0 at +-delta."""
    if n < 3:
        return torch.randn(G, C, n, generator=g, dtype=F64)
    assert delta * delta < n - 1, "delta <= sqrt(n - 1)"
    r = torch.randn(G, C, n - 1, generator=g, dtype=F64)
    r = r - r.mean(-1, keepdim=True)
    r = r / r.square().mean(-1, keepdim=True).sqrt()
    s = torch.where(torch.rand(G, C, 1, generator=g, dtype=F64) < 0.5, -1.0, 1.0) * delta
    m = -s / (n - 1)
    sd = ((n - delta * delta) / (n - 1) - m * m).sqrt()
    return torch.cat([s, m + sd * r], -1)


def _pool_windows(t, fill):
    """[N,C,H,W] -> [N*C, 9, Ho*Wo] windows of the 3x3 / 2 / 1 pooling, `fill` outside the map."""
    N, C, H, W = t.shape
    return F.unfold(F.pad(t.reshape(N * C, 1, H, W), (1, 1, 1, 1), value=fill), 3, stride=2)


def pool_gap(z):
    """Winner minus runner-up of relu(z) in every pooling window, [N*C, Ho*Wo]."""
    top = _pool_windows(torch.relu(z), -1.0).topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


@lru_cache(maxsize=4)
def make(shape, groups=1, kind="bulk", kappa=0.3, delta=1.0, relu=True, with_res=False, training=True, pool=False, track=True, seed=0):
    N, C, H, W = shape
    G, n = groups, (N // groups) * H * W
    g = torch.Generator().manual_seed(7919 * seed + 31 * C + N + 1000 * G + 17 * len(kind) + int(kappa) + int(delta))
    sigma = 1.7 * (0.5 + 1.5 * torch.rand(C, generator=g, dtype=F64))                      # per channel
    fg = torch.linspace(0.7, 1.4, G, dtype=F64) if G > 1 else torch.ones(1, dtype=F64)     # per group
    sign = torch.where(torch.rand(C, generator=g, dtype=F64) < 0.5, -1.0, 1.0)
    sd = fg[:, None] * sigma[None]                                                         # [G,C]
    mu = kappa * sd * sign[None]
    u = _standardised(g, G, C, n, delta)
    b = mu[..., None] + sd[..., None] * u
    sp = SPECIAL if C > SPECIAL else 0
    if kind == "flat":
        b[:, sp] = 1.0
    elif kind == "tiny_var":
        b[:, sp] = 1.0 + 1e-4 * u[:, sp]
        sigma[sp], sd[:, sp] = 1e-4, 1e-4
    x = _unblocks(b, shape, G).to(F32)
    gamma = (0.5 + torch.rand(C, generator=g, dtype=F64)) * torch.where(torch.rand(C, generator=g, dtype=F64) < 0.25, -1.0, 1.0)
    beta = torch.randn(C, generator=g, dtype=F64) * 0.3
    beta = torch.where(beta < 0, beta - 0.05, beta + 0.05)
    if delta > 16:
        # the output scale is the outlier's (~ delta * gamma), so the kink band of 1e-3 of it is half a standard deviation of everything
        # else (0.45 sigma): a bias of two keeps the bulk of every channel on one side of the kink instead of nudging a third of it
        beta = torch.where(beta < 0, beta - 2.0, beta + 2.0)
    if C > NEG:
        gamma[NEG] = -gamma[NEG].abs()
    if C > ZERO and not pool:
        gamma[ZERO] = 0.0
    gamma[sp], beta[sp] = gamma[sp].abs(), beta[sp].abs() + 0.2
    if kind == "tiny_var":
        gamma[sp] = 31.6            # sigma = 1e-4 under eps = 1e-5: rstd is 316, not 1e4; this gamma brings the channel's output back to O(1)
    centre = mu.mean(0) if kind not in ("flat", "tiny_var") else torch.where(torch.arange(C) == sp, 1.0, mu.mean(0))
    rm0 = (centre + 0.2 * sigma * torch.randn(C, generator=g, dtype=F64)).to(F32)
    rv0 = (sigma.square() * (0.5 + torch.rand(C, generator=g, dtype=F64))).to(F32)
    gamma, beta = gamma.to(F32), beta.to(F32)
    res = torch.randn(shape, generator=g, dtype=F64).to(F32) if with_res else None
    oshape = (N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1) if pool else shape
    cot = torch.randn(oshape, generator=g, dtype=F64).to(F32)
    step = (0.06 * sigma).view(1, C, 1, 1) * torch.sign(gamma.double() + 1e-30).view(1, C, 1, 1)
    first = torch.zeros(shape, dtype=torch.bool)
    first[::N // G, :, 0, 0] = True
    stats_from_batch = training or not track
    for _ in range(40):
        with torch.no_grad():
            y, z, _, rstd, _, _ = forward64(x.double(), res.double() if with_res else None, gamma.double(), beta.double(), rm0.double(),
                                            rv0.double(), stats_from_batch, G, relu, pool)
        scale = float(y.abs().max())
        ok = True
        if relu:
            near = z.abs() < 2 * KINK * scale
            if bool(near.any()):
                ok = False
                if with_res:
                    res = torch.where(near, res.double() + 0.05, res.double()).to(F32)
                else:
                    x = torch.where(near, x.double() + step * torch.where(z < 0, -1.0, 1.0), x.double()).to(F32)
        if pool and ok:
            # windows whose winner does not lead by 2e-3 of the scale: lift one element of the window (never x_first) clear of the rest
            zw = _pool_windows(z, -1e300)
            pos = _pool_windows(torch.arange(N * C * H * W, dtype=F64).view(shape), -1.0)
            cand = _pool_windows(torch.where(first, torch.full_like(z, -1e300), z), -1e300)
            bad = pool_gap(z) < 2 * KINK * scale
            if kind == "flat":
                bad = bad & (torch.arange(N * C) % C != sp)[:, None]
            if bool(bad.any()):
                ok = False
                w = cand.argmax(1)                                                  # [N*C, L]
                tgt = pos.gather(1, w[:, None])[:, 0][bad].long()
                need = (zw.max(1).values.clamp_min(0.0) - cand.max(1).values)[bad]
                c_of = (tgt // (H * W)) % C
                g_of = (tgt // (C * H * W)) // (N // G)
                slope = (gamma.double()[c_of] * rstd[g_of, c_of]).abs()
                dx = torch.sign(gamma.double()[c_of]) * (need / slope + 0.3 * sd[g_of, c_of])
                xf = x.double().view(-1)
                xf[tgt] = xf[tgt] + dx
                x = xf.view(shape).to(F32)
        if ok:
            break
    else:
        raise AssertionError("the case generator did not settle: %r" % ((shape, groups, kind, kappa, delta),))
    return Case(shape=shape, groups=groups, kind=kind, kappa=kappa, delta=delta, relu=relu, with_res=with_res, training=training, pool=pool,
                track=track, special=sp, x=x.contiguous(), res=res, cot=cot, gamma=gamma, beta=beta, rm0=rm0 if track else None,
                rv0=rv0 if track else None)


QUANTITIES = ("y", "dx", "dres", "dgamma", "dbeta", "running_mean", "running_var", "save_mean", "save_rstd")


@lru_cache(maxsize=4)
def reference(case):
    """float64: y, z, the gradients of <y, cot>, the running statistics after the call, the saved statistics."""
    c, dt = case, F64
    x = c.x.to(dt).requires_grad_(True)
    res = c.res.to(dt).requires_grad_(True) if c.with_res else None
    gamma, beta = c.gamma.to(dt).requires_grad_(True), c.beta.to(dt).requires_grad_(True)
    training = c.training or not c.track
    rm = c.rm0.to(dt) if c.rm0 is not None else None
    rv = c.rv0.to(dt) if c.rv0 is not None else None
    y, z, sm, sr, rm, rv = forward64(x, res, gamma, beta, rm, rv, training, c.groups, c.relu, c.pool)
    leaves = [x, gamma, beta] + ([res] if c.with_res else [])
    gs = torch.autograd.grad((y * c.cot.to(dt)).sum(), leaves)
    out = dict(y=y.detach(), z=z.detach(), dx=gs[0], dgamma=gs[1], dbeta=gs[2], save_mean=sm, save_rstd=sr)
    if c.with_res:
        out["dres"] = gs[3]
    if rm is not None and training:
        out["running_mean"], out["running_var"] = rm, rv
    return out
