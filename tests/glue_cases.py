"""Seeded inputs and float64 / fp32 references of the one-launch glue kernels (csrc/camera.hip, transform_normal of csrc/camera_prior.hip,
csrc/latent_bias.hip, csrc/loss.hip).  Plain module, no GPU: tests/test_glue_cases_host.py checks the cases' preconditions on the CPU,
tests/test_gpu_glue_float64.py compares the kernels with the references.

Every generator draws fp32 inputs and cotangents from one seeded CPU generator.  Every reference evaluates the operation and its
gradients by autograd through oracle/reference_ops.py under R.default_dtype(dt), dt fp32 or float64, on FRESH leaves built from the fp32
inputs (t.to(float32) returns the same tensor: a leaf made from it a second time would no longer be one)."""
import math
from contextlib import contextmanager, nullcontext
from functools import lru_cache

import torch
import torch.nn.functional as F

from oracle import reference_ops as R

DTYPES = (torch.float32, torch.float64)


def _leaf(t, dt):
    return t.detach().to(dt).clone().requires_grad_(True)


def _grads(f, leaves):
    """d f / d leaves; a leaf the functional does not reach has gradient zero."""
    gs = torch.autograd.grad(f, leaves, allow_unused=True)
    return [(g if g is not None else torch.zeros_like(v)).detach() for g, v in zip(gs, leaves)]


def _dot(outs, cots, dt):
    return sum((o * c.to(dt)).sum() for o, c in zip(outs, cots) if c is not None)


# ---------------------------------------------------------------------------------------------------------------------------------
# camera_rays
# ---------------------------------------------------------------------------------------------------------------------------------
# (B, R, H, W, sampled, t_z): one block of 256 threads per image, so R = 63 / 64 (one wave), 257 (a second trip of one thread), 512 (two
# full trips), B = 65 (many blocks); far: the reference's (R^T g + t_inv) - t_inv cancels against t_inv ~ 50.
CAMERA_CASES = {
    "1x1_8x8": (1, 1, 8, 8, True, 5.0),
    "2x63_16x24": (2, 63, 16, 24, True, 5.0),
    "2x64_16x24": (2, 64, 16, 24, True, 5.0),
    "3x257_16x24": (3, 257, 16, 24, True, 5.0),
    "3x512_224x224": (3, 512, 224, 224, True, 5.0),
    "65x32_8x8": (65, 32, 8, 8, True, 5.0),
    "2x64_8x8_all_pixels": (2, 64, 8, 8, False, 5.0),
    "2x64_16x24_far": (2, 64, 16, 24, True, 50.0),
}
CAMERA_OUTPUTS = ("cam_loc", "ray_dirs", "depth_fac")
CAMERA_SUBSETS = {"all": CAMERA_OUTPUTS, "cam_loc": ("cam_loc",), "ray_dirs": ("ray_dirs",), "depth_fac": ("depth_fac",)}


def random_pose(B, t_z, g):
    """[B,3,4]: a random rotation and a translation around (0, 0, t_z)."""
    q = torch.linalg.qr(torch.randn(B, 3, 3, generator=g))[0]
    t = torch.randn(B, 3, 1, generator=g) * 0.3 + torch.tensor([0.0, 0.0, t_z]).view(1, 3, 1)
    return torch.cat([q, t], dim=-1).contiguous()


def planted_ray_idx(B, n, H, W, g):
    """int64 [B,n] pixel indices: a random draw, then the four image corners (rotated per image) in the first slots and one repeated
    index, as far as n has room for them."""
    idx = torch.stack([torch.randperm(H * W, generator=g)[:n] for _ in range(B)])
    corners = [0, W - 1, (H - 1) * W, H * W - 1]
    for b in range(B):
        for k in range(min(n, 4)):
            idx[b, k] = corners[(k + b) % 4]
        if n >= 6:
            idx[b, 5] = idx[b, 4]
    return idx


@lru_cache(maxsize=None)
def camera_inputs(case):
    B, n, H, W, sampled, t_z = CAMERA_CASES[case]
    g = torch.Generator().manual_seed(1000 + sorted(CAMERA_CASES).index(case))
    cfg = R.Cfg(H=H, W=W)
    pose = random_pose(B, t_z, g)
    intr = R.get_intr(cfg, 1 + 0.1 * torch.randn(B, generator=g))
    intr[:, 0, 1] = 0.01 * W                      # skew: the full inverse of K is exercised
    intr[:, 1, 1] *= 1.07                         # f W != f H at square images too
    ray_idx = planted_ray_idx(B, n, H, W, g) if sampled else None
    cot = dict(cam_loc=torch.randn(B * n, 3, generator=g), ray_dirs=torch.randn(B * n, 3, generator=g),
               depth_fac=torch.randn(B * n, generator=g))
    return dict(cfg=cfg, B=B, R=n, W=W, pose=pose, intr=intr.contiguous(), ray_idx=ray_idx, cot=cot)


def camera_rays_ops(cfg, pose, intr, ray_idx, n):
    """cam_loc [B*n,3], ray_dirs [B*n,3], depth_fac [B*n] as R.render sets a render's rays up."""
    center, ray = R.get_center_and_ray(cfg, pose, intr)
    B = pose.shape[0]
    ray = ray.gather(1, ray_idx[..., None].expand(B, n, 3)) if ray_idx is not None else ray[:, :n]
    d = F.normalize(ray, dim=-1)
    df = d.norm(dim=-1, keepdim=True) / ray.norm(dim=-1, keepdim=True)
    return center.expand(B, n, 3).reshape(-1, 3), d.reshape(-1, 3), df.reshape(-1)


@lru_cache(maxsize=None)
def camera_reference(case, subset, dt):
    """{cam_loc, ray_dirs, depth_fac, d_pose, d_intr}: the gradients of sum_k <output_k, cotangent_k> over the outputs in subset."""
    c = camera_inputs(case)
    with R.default_dtype(dt):
        pose, intr = _leaf(c["pose"], dt), _leaf(c["intr"], dt)
        outs = camera_rays_ops(c["cfg"], pose, intr, c["ray_idx"], c["R"])
        f = _dot(outs, [c["cot"][k] if k in CAMERA_SUBSETS[subset] else None for k in CAMERA_OUTPUTS], dt)
        gp, gk = _grads(f, [pose, intr])
    return dict(zip(CAMERA_OUTPUTS, [o.detach() for o in outs]), d_pose=gp, d_intr=gk)


# ---------------------------------------------------------------------------------------------------------------------------------
# pose_from_trig
# ---------------------------------------------------------------------------------------------------------------------------------
TRIG_B = (1, 5, 64, 65, 200)                     # 64 threads per block: one thread, a partial block, a full one, a second one, four
TRIG_W, TRIG_H = 64, 48
TRIG_LEAVES = ("azim", "elev", "theta", "scale_focal", "scale_dist")
TRIG_SUBSETS = {"both": ("pose", "intr"), "pose": ("pose",), "intr": ("intr",)}


@lru_cache(maxsize=None)
def trig_inputs(B, unit=False):
    """(cos, sin) pairs that are deliberately NOT unit (norms 0.3 .. 2): the formulas are polynomial in c and s."""
    g = torch.Generator().manual_seed(2000 + B)
    pair = lambda: F.normalize(torch.randn(B, 2, generator=g), dim=1) * (1.0 if unit else 0.3 + 1.7 * torch.rand(B, 1, generator=g))
    leaves = dict(azim=pair(), elev=pair(), theta=pair(), scale_focal=1 + 0.2 * torch.randn(B, generator=g),
                  scale_dist=1 + 0.2 * torch.randn(B, generator=g))
    cot = dict(pose=torch.randn(B, 3, 4, generator=g), intr=torch.randn(B, 3, 3, generator=g))
    return dict(cfg=R.Cfg(H=TRIG_H, W=TRIG_W), leaves=leaves, cot=cot)


def trig_ops(cfg, azim, elev, theta, scale_focal, scale_dist):
    return R.pose_from_trig(cfg, azim, elev, theta, scale_dist), R.get_intr(cfg, scale_focal)


@lru_cache(maxsize=None)
def trig_reference(B, subset, dt):
    c = trig_inputs(B)
    with R.default_dtype(dt):
        leaves = [_leaf(c["leaves"][k], dt) for k in TRIG_LEAVES]
        pose, intr = trig_ops(c["cfg"], *leaves)
        f = _dot((pose, intr), [c["cot"][k] if k in TRIG_SUBSETS[subset] else None for k in ("pose", "intr")], dt)
        gs = _grads(f, leaves)
    return dict(pose=pose.detach(), intr=intr.detach(), **{"d_" + k: g for k, g in zip(TRIG_LEAVES, gs)})


# ---------------------------------------------------------------------------------------------------------------------------------
# transform_normal
# ---------------------------------------------------------------------------------------------------------------------------------
NORMAL_CASES = ((1, 1), (2, 255), (3, 257), (4, 512), (2, 1000))      # 256 threads per block: below, across and several trips


@lru_cache(maxsize=None)
def normal_inputs(B, n):
    g = torch.Generator().manual_seed(3000 + 7 * B + n)
    return dict(normals=F.normalize(torch.randn(B, n, 3, generator=g), dim=-1), pose=torch.randn(B, 3, 4, generator=g),   # not orthonormal
                cot=torch.randn(B, n, 3, generator=g))


@lru_cache(maxsize=None)
def normal_reference(B, n, dt):
    c = normal_inputs(B, n)
    with R.default_dtype(dt):
        pose = _leaf(c["pose"], dt)
        out = R.transform_normal(c["normals"].to(dt), pose)
        gp, = _grads(_dot((out,), (c["cot"],), dt), [pose])
    return dict(out=out.detach(), d_pose=gp)


# ---------------------------------------------------------------------------------------------------------------------------------
# latent bias: c[b][l] = bias[l] + (l < L ? post[l] * lat[l] z[b] : 0)
# ---------------------------------------------------------------------------------------------------------------------------------
# (B, Z, L, NL, post): B = 9 / 33 leave a remainder of the unroll by 8; Z = 300 > 256 takes a second trip of the 256-thread loops and is
# no multiple of 4; Z = 7 is smaller than everything.
LATENT_CASES = ((1, 64, 3, 5, True), (1, 64, 1, 3, False), (9, 64, 3, 5, True), (33, 64, 1, 3, False), (2, 300, 3, 5, True),
                (4, 256, 3, 5, True), (3, 7, 3, 5, True))
LATENT_POST = (1.0, 1.0 / math.sqrt(2.0), 0.37)      # distinct per layer: a swapped or dropped factor shows


@lru_cache(maxsize=None)
def latent_inputs(B, Z, L, NL, with_post):
    g = torch.Generator().manual_seed(4000 + 131 * B + Z + L)
    return dict(z=torch.randn(B, Z, generator=g), lat=torch.randn(L * 64, Z, generator=g) / math.sqrt(Z), bias=torch.randn(NL, 64, generator=g),
                post=torch.tensor(LATENT_POST[:L]) if with_post else None, cot=torch.randn(B, NL, 64, generator=g))


def latent_ops(z, lat, bias, post):
    """The host branch of packing._bias_from."""
    B, L, NL = z.shape[0], lat.shape[0] // 64, bias.shape[0]
    zw = (z @ lat.t()).view(B, L, 64)
    if post is not None:
        zw = zw * post.to(zw.dtype).view(1, L, 1)
    return F.pad(zw, (0, 0, 0, NL - L)) + bias.unsqueeze(0)


@lru_cache(maxsize=None)
def latent_reference(B, Z, L, NL, with_post, dt):
    c = latent_inputs(B, Z, L, NL, with_post)
    with R.default_dtype(dt):
        z, lat, bias = _leaf(c["z"], dt), _leaf(c["lat"], dt), _leaf(c["bias"], dt)
        out = latent_ops(z, lat, bias, c["post"])
        gz, gl, gb = _grads(_dot((out,), (c["cot"],), dt), [z, lat, bias])
    return dict(out=out.detach(), g_z=gz, g_lat=gl, g_bias=gb)


# ---------------------------------------------------------------------------------------------------------------------------------
# fused losses
# ---------------------------------------------------------------------------------------------------------------------------------
# (B, R, E | None, mask_mse, tolerance): 16 x 1024 is exactly the register-resident 16,384 rays of the selection, 17 x 1024 just past it.
LOSS_CASES = {
    "1x1x1": (1, 1, 1, 0.3, 0.2),                    # one masked ray: n_keep = int(0.8) = 0, the normal loss is NaN
    "2x64x64": (2, 64, 64, 0.0, 0.0),
    "2x64_no_eik": (2, 64, None, 0.3, 0.0),
    "3x100x37": (3, 100, 37, 0.3, 0.5),              # image 0: target and prediction all zero; image 1: fully covered
    "5x333x77": (5, 333, 77, 0.3, 0.2),              # exact duplicates planted across the rank-n_keep boundary
    "16x1024x1024": (16, 1024, 1024, 0.0, 0.2),
    "17x1024x8": (17, 1024, 8, 0.3, 0.5),
}
LOSS_WEIGHTS = (1.0, 0.5, 0.01, 0.03)                # render, mask, normal, eikonal
LOSS_LEAVES = ("rgb", "mask", "normal", "normal_t", "eik")
LOSS_VALUES = ("render", "mask", "normal", "eikonal")
LOSS_SUBSETS = {"all": LOSS_WEIGHTS, "normal_only": (0.0, 0.0, 1.0, 0.0)}
N_PLANTED = 5


def _angular64(c):
    """(flat indices of the masked rays, their float64 angular errors)."""
    m = ((c["mask_t"] > 0.5) & (c["mask"] > 0.5)).view(-1)
    ang = 1 - (c["normal"].double() * c["normal_t"].double()).sum(-1).view(-1)
    idx = torch.nonzero(m).view(-1)
    return idx, ang[idx]


def n_keep_of(n, tol):
    return int(n * (1 - tol))


@lru_cache(maxsize=None)
def loss_inputs(case):
    B, n, E, mask_mse, tol = LOSS_CASES[case]
    g = torch.Generator().manual_seed(5000 + sorted(LOSS_CASES).index(case))
    unit = lambda: F.normalize(torch.randn(B, n, 3, generator=g), dim=-1)
    c = dict(rgb=torch.rand(B, n, 3, generator=g), rgb_t=torch.rand(B, n, 3, generator=g), mask=torch.rand(B, n, 1, generator=g),
             mask_t=(torch.rand(B, n, 1, generator=g) > 0.4).float(), normal=unit(), normal_t=unit(),
             eik=(0.5 + torch.rand(B * E, generator=g)) if E is not None else None, planted=())
    if case == "1x1x1":
        c["mask"][:], c["mask_t"][:] = 0.8, 1.0
    if case == "3x100x37":
        c["mask"][0], c["mask_t"][0] = 0.0, 0.0                                        # the union is the 1e-8 terms alone
        c["mask"][1], c["mask_t"][1] = 0.5 + 0.5 * c["mask"][1].clamp(min=0.01), 1.0   # fully covered: every ray of it is masked in
    if case == "5x333x77":
        # the ray at rank n_keep, copied over the N_PLANTED masked rays with the largest error: N_PLANTED + 1 exact ties of which one is
        # kept -- the one with the lowest index, as a stable sort keeps it
        idx, ang = _angular64(c)
        order = torch.argsort(ang, stable=True)
        src = idx[order[n_keep_of(len(idx), tol) - 1]]
        dst = idx[order[-N_PLANTED:]]
        for k in ("normal", "normal_t"):
            flat = c[k].view(-1, 3)
            flat[dst] = flat[src].clone()
        c["planted"] = tuple(sorted([int(src)] + [int(d) for d in dst]))
    c.update(B=B, R=n, E=E, cfg=R.Cfg(mask_mse=mask_mse), mask_mse=mask_mse, tol=tol)
    return c


@contextmanager
def stable_sort():
    """torch.sort leaves the order of equal keys open (on 5x333x77 the CPU sort keeps neither the first nor the last of the planted
    ties), so WHICH of several exact ties at rank n_keep is kept is not defined by R.normal_loss.  The kernel keeps the lowest indices,
    that is the order of a stable sort: the reference is evaluated in that order.  Without ties this changes nothing
    (test_glue_cases_host.py)."""
    real = torch.sort
    torch.sort = lambda *a, **k: real(*a, **dict(k, stable=True))
    try:
        yield
    finally:
        torch.sort = real


def loss_ops(cfg, rgb, rgb_t, mask, mask_t, normal, normal_t, eik, tol, stable=True):
    """The four losses of one render as model/loss.py computes them."""
    m = (mask_t > 0.5) & (mask > 0.5)
    with stable_sort() if stable else nullcontext():
        normal_loss = R.normal_loss(cfg, normal, normal_t, m, tolerance=tol)
    return (R.mse_loss(rgb, rgb_t), R.mask_loss(cfg, mask, mask_t), normal_loss,
            R.mse_loss(eik, 1.0) if eik is not None else torch.zeros((), dtype=rgb.dtype))


def kept_rays(c, stable=True):
    """[B*R] bool: the rays R.normal_loss keeps (those that get a gradient), float64."""
    with R.default_dtype(torch.float64):
        n = _leaf(c["normal"], torch.float64)
        m = (c["mask_t"] > 0.5) & (c["mask"] > 0.5)
        with stable_sort() if stable else nullcontext():
            f = R.normal_loss(c["cfg"], n, c["normal_t"].double(), m, tolerance=c["tol"])
        g, = _grads(torch.nan_to_num(f), [n])
    return (g.abs().sum(-1) != 0).view(-1)


@lru_cache(maxsize=None)
def loss_reference(case, subset, dt):
    """{render, mask, normal, eikonal, g_rgb, g_mask, g_normal, g_normal_t, g_eik} for the weighted sum of the losses in subset."""
    c = loss_inputs(case)
    w = LOSS_SUBSETS[subset]
    with R.default_dtype(dt):
        leaves = {k: _leaf(c[k], dt) for k in LOSS_LEAVES if c[k] is not None}
        vals = loss_ops(c["cfg"], leaves["rgb"], c["rgb_t"].to(dt), leaves["mask"], c["mask_t"].to(dt), leaves["normal"], leaves["normal_t"],
                        leaves.get("eik"), c["tol"])
        f = sum(wk * v for wk, v in zip(w, vals) if wk != 0.0 and v.requires_grad)
        gs = _grads(f, list(leaves.values()))
    out = dict(zip(LOSS_VALUES, [v.detach() for v in vals]))
    out.update({"g_" + k: g for k, g in zip(leaves, gs)})
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# chain: unit trig pairs -> pose_from_trig -> camera_rays (100 sampled rays at 16 x 24) and transform_normal
# ---------------------------------------------------------------------------------------------------------------------------------
CHAIN = dict(B=3, R=100, H=16, W=24)
CHAIN_OUTPUTS = CAMERA_OUTPUTS + ("normal_t",)


@lru_cache(maxsize=None)
def chain_inputs():
    B, n, H, W = CHAIN["B"], CHAIN["R"], CHAIN["H"], CHAIN["W"]
    g = torch.Generator().manual_seed(6000)
    t = trig_inputs(B, unit=True)
    cot = dict(cam_loc=torch.randn(B * n, 3, generator=g), ray_dirs=torch.randn(B * n, 3, generator=g), depth_fac=torch.randn(B * n, generator=g),
               normal_t=torch.randn(B, n, 3, generator=g))
    return dict(cfg=R.Cfg(H=H, W=W), leaves=t["leaves"], ray_idx=planted_ray_idx(B, n, H, W, g),
                normals=F.normalize(torch.randn(B, n, 3, generator=g), dim=-1), cot=cot)


@lru_cache(maxsize=None)
def chain_reference(dt):
    c = chain_inputs()
    with R.default_dtype(dt):
        leaves = [_leaf(c["leaves"][k], dt) for k in TRIG_LEAVES]
        pose, intr = trig_ops(c["cfg"], *leaves)
        outs = camera_rays_ops(c["cfg"], pose, intr, c["ray_idx"], CHAIN["R"]) + (R.transform_normal(c["normals"].to(dt), pose),)
        gs = _grads(_dot(outs, [c["cot"][k] for k in CHAIN_OUTPUTS], dt), leaves)
    return dict(zip(CHAIN_OUTPUTS, [o.detach() for o in outs]), **{"d_" + k: g for k, g in zip(TRIG_LEAVES, gs)})
