"""VolSDF-style volume renderer of the MI355X build.

Call surface = reference model/renderer.py:  Renderer(opt, sdf_network, rgb_network) and
forward(opt, pose, intr, scale_dist, proj_latent_sdf, proj_latent_rgb, ray_idx=None, training=True,
visualize=False) -> 6-tuple (9-tuple with visualize).  What differs is where the work happens:

  reference                                   this build
  ---------                                   ----------
  all H*W rays, then gather(ray_idx)          rays only for the rendered pixels (utils/camera.py)
  ~40 torch ops / ~40 KB of temporaries       3 fused HIP kernels per render, ~0.6 KB/pt of HBM traffic
  per sample point, autograd double backward  hand-derived backward kernels (sdf_bwd / rgb_bwd / wgrad)

Random numbers: exactly the reference's CPU-generator draws, in its order (rand [BR,64] -> randint
[BR] -> uniform_ [BR,3]; renderer.py:29,33,158), so a seeded run consumes the same stream.
"""
from __future__ import annotations

import collections

import torch
import torch.nn as nn
import torch.nn.functional as torch_F

from .. import ops
from ..functional import CameraRaysFunction, RaySampleEikFunction, RaySampleFunction, RgbCompositeFunction, SdfFunction
from ..utils import camera, options
from .implicit import LaplaceDensity


# render.n_samples_uniform values the HIP render kernels take (pure host logic; importing ops loads no library); any other value renders
# on model/eager_path.py
sample_count_supported = ops.sample_count_supported

UPLOAD_STREAM = True          # `--hip.upload_stream!`: the CPU-generator draws are copied in the render's own stream
_upload_streams = {}
VIEWS_MAX_RAYS = 128 * 128 * 32   # rays per pass of render_views: the evaluation render of tools/workloads.py render_eval_128


def _upload(x, dev):
    """Pinned host tensor -> device on the device's upload stream; the current stream waits for it (an event, no host wait)."""
    main = torch.cuda.current_stream(dev)
    side = _upload_streams.get(dev.index)
    if side is None:
        side = _upload_streams[dev.index] = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        d = x.to(dev, non_blocking=True)        # the pinned block is held by the host allocator until this copy has run
    main.wait_stream(side)
    d.record_stream(main)                       # allocated on the upload stream, used on the render's
    return d


SurfaceRender = collections.namedtuple("SurfaceRender", ["rgb", "mask", "depth", "normal", "hit"])
SURFACE_REFINE_MAX = 16       # `--hip.surface_refine` 0..16
SURFACE_SCALE_MAX = 4         # `--hip.surface_scale` 1..4


class UniformSampler(nn.Module):
    """Stratified depth samples in [dist*s - 0.7, dist*s + 0.7] (reference model/renderer.py:8-37)."""

    def __init__(self, opt):
        super().__init__()
        self.N_samples = opt.render.n_samples_uniform

    def get_z_vals(self, opt, ray_dirs, scale_dist, training=True):
        n_total = ray_dirs.shape[0]
        dev = ray_dirs.device
        n_rays = n_total // scale_dist.shape[0]
        centre = (opt.camera.dist * scale_dist).repeat_interleave(n_rays).view(n_total, 1)
        near, far = centre - 0.7, centre + 0.7
        t = torch.linspace(0.0, 1.0, steps=self.N_samples).to(dev)
        z_vals = near * (1.0 - t) + far * t
        if training:
            mids = 0.5 * (z_vals[..., 1:] + z_vals[..., :-1])
            upper = torch.cat([mids, z_vals[..., -1:]], -1)
            lower = torch.cat([z_vals[..., :1], mids], -1)
            t_rand = torch.rand(z_vals.shape).to(dev)              # CPU generator, as the reference
            z_vals = lower + (upper - lower) * t_rand
        idx = torch.randint(z_vals.shape[-1], (n_total,)).to(dev)  # CPU generator
        return z_vals, torch.gather(z_vals, 1, idx.unsqueeze(-1))


class Renderer(nn.Module):

    def __init__(self, opt, sdf_network, rgb_network):
        super().__init__()
        self.bg_color = float(opt.data.bgcolor)
        self.eik_range = opt.arch.impl_sdf.eikonal_sample_range
        self.normal_model = opt.render.normal_model
        self.sdf_network = sdf_network
        self.rgb_network = rgb_network
        self.density = LaplaceDensity(params_init={"beta": opt.arch.impl_sdf.beta_init})
        if opt.render.sampler != "uniform":
            raise NotImplementedError(opt.render.sampler)
        if self.normal_model != "volume":
            raise NotImplementedError("only render.normal_model=volume is implemented (the shipped setting)")
        self.ray_sampler = UniformSampler(opt)
        self.N_samples = opt.render.n_samples_uniform
        # The render kernels walk a ray in chunks of 64 samples (one 64-lane wavefront per ray) and the chain kernels hold one architecture
        # family in LDS: a render.n_samples_uniform outside sample_count_supported or other arch.impl_* run on stock device operators
        # (model/eager_path.py, round 5).
        supported = sample_count_supported(self.N_samples)
        self.eager = bool(getattr(sdf_network, "eager", False) or getattr(rgb_network, "eager", False) or not supported)
        if self.eager:
            from . import eager_path
            eager_path.warn_once("render.n_samples_uniform = %d" % self.N_samples if not supported else "implicit networks")
            sdf_network.eager = rgb_network.eager = True          # one path for the whole render (the HIP kernels hand TBL64 features to each other)

    def forward(self, opt, pose, intr, scale_dist, proj_latent_sdf, proj_latent_rgb, ray_idx=None, training=True,
                visualize=False):
        S = self.N_samples
        sym = bool(self.sdf_network.force_symmetry)
        if opt.camera.model == "perspective" and pose.is_cuda:
            # one launch: pixel centres -> K^-1 -> camera-to-world -> unit rays + depth factor (csrc/camera.hip)
            B = pose.shape[0]
            R = ray_idx.shape[1] if ray_idx is not None else opt.H * opt.W
            cam_loc, ray_dirs, depth_fac = CameraRaysFunction.apply(pose, intr, ray_idx, R, int(opt.W))
        else:
            cam_loc, ray_raw = camera.get_center_and_ray(opt, pose, intr=intr, device=pose.device, ray_idx=ray_idx)
            ray_dirs = torch_F.normalize(ray_raw, dim=-1)
            depth_fac = ray_dirs.norm(dim=-1, keepdim=True) / ray_raw.norm(dim=-1, keepdim=True)
            B, R, _ = ray_dirs.shape
            if opt.camera.model == "perspective":
                cam_loc = cam_loc.expand(B, R, 3)
            cam_loc = cam_loc.reshape(-1, 3)
            ray_dirs = ray_dirs.reshape(-1, 3)
            depth_fac = depth_fac.reshape(-1)

        # reference CPU-generator draws, in its order (renderer.py:29,33): jitter then the eikonal sample index
        dev_rng = bool(options.hip(opt, "device_rng"))       # True: draw on the GPU (no 4 MB H2D copy per render,
        rdev = ray_dirs.device if dev_rng else "cpu"         # but a different random stream than the reference)
        # CPU draws land in pinned memory and are copied asynchronously: a pageable H2D copy would drain the stream
        # (one host sync per draw, three per render) and let the GPU idle while the host catches up.
        pin = (not dev_rng) and ray_dirs.is_cuda
        # ... and they travel on an UPLOAD stream of their own (round 5): the host is milliseconds ahead of the GPU when it reaches a render, so
        # the 4 MB of jitter are on the device long before the render's stream gets there -- in that stream the copy was ~100 us per render
        # with nothing else running (`--hip.upload_stream!`: copy in the render's stream)
        if pin and UPLOAD_STREAM:
            up = lambda x: _upload(x, ray_dirs.device)
        else:
            up = lambda x: x.to(ray_dirs.device, non_blocking=True)
        t_rand = up(torch.rand(B * R, S, device=rdev, pin_memory=pin)) if training else None
        eik_idx = up(torch.randint(S, (B * R,), device=rdev, pin_memory=pin))
        if self.eager:
            return self._forward_eager(opt, cam_loc, ray_dirs, depth_fac, scale_dist, t_rand, eik_idx, B, R, proj_latent_sdf, proj_latent_rgb,
                                       training, visualize, up, rdev, pin)
        eik_points = None
        if training and ray_dirs.is_cuda:
            # the eikonal points come out of the sampling launch: the uniform draw (CPU generator, the reference's third draw of a render,
            # renderer.py:158 -- nothing else touches the generator in between) and, per ray, the sample eik_idx as its near-surface point
            eik_u = up(torch.empty(B * R, 3, device=rdev, pin_memory=pin).uniform_(self.eik_range[0], self.eik_range[1]))
            z_vals, points_flat, eik_points = RaySampleEikFunction.apply(cam_loc, ray_dirs, scale_dist, t_rand, eik_idx, eik_u, R, float(opt.camera.dist))
        else:
            z_vals, points_flat = RaySampleFunction.apply(cam_loc, ray_dirs, scale_dist, t_rand, R, float(opt.camera.dist), S)
            z_eik = torch.gather(z_vals, 1, eik_idx.unsqueeze(-1))
        assert proj_latent_rgb.shape[1] == opt.arch.impl_rgb.proj_latent_dim

        # fused SDF value + feature + d(sdf)/dx, then RGB MLP + density + compositing
        w_pack, cbias = self.sdf_network.packed(proj_latent_sdf)
        fused_bwd = bool(options.hip(opt, "fused_backward"))
        sdf, grad, feat = SdfFunction.apply(points_flat, w_pack, cbias, R * S, sym, True, True, fused_bwd)
        v_pack, dbias = self.rgb_network.packed(proj_latent_rgb)
        outs = RgbCompositeFunction.apply(points_flat, z_vals, depth_fac.contiguous(), sdf, grad, feat,
                                          v_pack, dbias, self.density.beta, R, sym, float(self.density.beta_min),
                                          self.bg_color, float(opt.reg.normal_pow), bool(visualize))
        rgb, mask, mask_hard, depth, normal = outs[:5]
        rgb_output = rgb.view(B, R, 3)
        mask_output = mask.view(B, R, 1)
        mask_hard_output = mask_hard.view(B, R, 1)
        depth_output = depth.view(B, R, 1)
        normal_output = normal.view(B, R, 3)

        grad_eikonal = None
        if training:
            # uniform points (CPU generator, as the reference) + one near-surface point per ray
            if eik_points is None:
                n_eik = B * R
                eik = up(torch.empty(n_eik, 3, device=rdev, pin_memory=pin).uniform_(self.eik_range[0], self.eik_range[1])).reshape(B, R, 3)
                near = (cam_loc + z_eik * ray_dirs).reshape(B, R, 3)
                eik_points = torch.cat([eik, near], 1)
            eik_points = eik_points.reshape(-1, 3)
            _, _, g_eik = self.sdf_network.get_conditional_output(opt, B, eik_points, proj_latent_sdf, compute_grad=True)
            grad_eikonal = g_eik.norm(2, dim=1)

        if visualize:
            weights, alphas, rgb_flat = outs[5:8]
            opacity = alphas.reshape(B, -1, 1)
            transp = torch.cat([opacity, 1 - opacity, torch.zeros_like(opacity)], dim=-1)
            rgba = torch.cat([rgb_flat.reshape(B, -1, 3), opacity], dim=-1)
            idx = torch.randperm(R)[:200].to(opacity.device)
            pick = lambda x: self.sample_rays_visualize(idx, x.reshape(B, R, S, -1))
            return (rgb_output, mask_output, mask_hard_output, depth_output, normal_output, grad_eikonal,
                    pick(points_flat.detach()), pick(transp), pick(rgba))
        return rgb_output, mask_output, mask_hard_output, depth_output, normal_output, grad_eikonal

    @torch.no_grad()
    def render_views(self, opt, poses, intr, proj_latent_sdf, proj_latent_rgb, max_rays=VIEWS_MAX_RAYS, chunk_views=None, surface=False,
                     n_refine=3, scale=1):
        """The B images (intr [B,3,3], latents [B,Z]) seen from each of V poses [V,3,4] with scale_dist 1 (the turn-table of
        reference runner.py:406-427) -> rgb [V,B,R,3], mask [V,B,R,1], normal [V,B,R,3], R = opt.H * opt.W, in as few passes of the chain
        CameraRaysFunction -> RaySampleFunction -> SdfFunction -> RgbCompositeFunction (training=False) as max_rays rays per pass allow, or
        chunk_views views per pass.  The views are laid out as extra images, view-major: image v*B + b has pose v and image b's intrinsics
        and per-image biases.  A ray's arithmetic does not depend on its batch neighbours, so the result equals the V renders of B images one
        at a time bit for bit.  Draws nothing from the random generators: Runner.vis_rotate makes the reference's draws.
        surface=True: the surface render of every view instead (render_surface with n_refine and scale, scale_dist 1) -> a SurfaceRender
        of rgb [V,B,R,3], mask, depth [V,B,R,1], normal [V,B,R,3], hit [V,B,R], R = scale^2 opt.H opt.W, laid out and batched the same
        way and equal to the V calls of render_surface bit for bit."""
        if self.eager or opt.camera.model != "perspective":
            raise NotImplementedError("render_views runs on the HIP render chain (perspective camera, compiled architecture and sample count)")
        V, B = poses.shape[0], intr.shape[0]
        if surface:
            k, n_refine, R = self._surface_args(opt, n_refine, scale)
            if chunk_views:
                per = int(chunk_views)
            else:
                per = max(1, int(max_rays) // (B * R))
                per = -(-V // -(-V // per))
            packs = self.sdf_network.packed(proj_latent_sdf) + self.rgb_network.packed(proj_latent_rgb)
            dev = poses.device
            out = SurfaceRender(*(torch.empty(V, B, R, c, device=dev) for c in (3, 1, 1, 3)), torch.empty(V, B, R, device=dev, dtype=torch.int32))
            ones = torch.ones(B, device=dev)
            for v0 in range(0, V, per):
                n = min(per, V - v0)
                pose = poses[v0:v0 + n].unsqueeze(1).expand(n, B, 3, 4).reshape(n * B, 3, 4)
                part = self._surface_chain(opt, pose, intr.repeat(n, 1, 1), ones.repeat(n), packs, B, n_refine, k, max_rays)
                for dst, src in zip(out, part):
                    dst[v0:v0 + n] = src.view(n, *dst.shape[1:])
            return out
        R, S = opt.H * opt.W, self.N_samples
        if chunk_views:
            per = int(chunk_views)
        else:
            per = max(1, int(max_rays) // (B * R))
            per = -(-V // -(-V // per))                 # the same number of passes, the views spread evenly over them
        sym = bool(self.sdf_network.force_symmetry)
        w_pack, cbias = self.sdf_network.packed(proj_latent_sdf)
        v_pack, dbias = self.rgb_network.packed(proj_latent_rgb)
        dev = poses.device
        rgb, mask, normal = (torch.empty(V, B, R, c, device=dev) for c in (3, 1, 3))
        for v0 in range(0, V, per):
            n = min(per, V - v0)
            pose = poses[v0:v0 + n].unsqueeze(1).expand(n, B, 3, 4).reshape(n * B, 3, 4)
            cam_loc, ray_dirs, depth_fac = CameraRaysFunction.apply(pose, intr.repeat(n, 1, 1), None, R, int(opt.W))
            ones = torch.ones(n * B, device=dev)
            z_vals, points_flat = RaySampleFunction.apply(cam_loc, ray_dirs, ones, None, R, float(opt.camera.dist), S)
            sdf, grad, feat = SdfFunction.apply(points_flat, w_pack, cbias.repeat(n, 1, 1), R * S, sym, True, True)
            outs = RgbCompositeFunction.apply(points_flat, z_vals, depth_fac.contiguous(), sdf, grad, feat, v_pack, dbias.repeat(n, 1, 1),
                                              self.density.beta, R, sym, float(self.density.beta_min), self.bg_color,
                                              float(opt.reg.normal_pow), False)
            rgb[v0:v0 + n] = outs[0].view(n, B, R, 3)
            mask[v0:v0 + n] = outs[1].view(n, B, R, 1)
            normal[v0:v0 + n] = outs[4].view(n, B, R, 3)
        return rgb, mask, normal

    def _surface_args(self, opt, n_refine, scale):
        """(scale, n_refine, rays per image) of a surface render, or the error it must raise -- before anything touches the device."""
        if self.eager or opt.camera.model != "perspective":
            raise NotImplementedError("render_surface runs on the HIP render chain (perspective camera, compiled architecture and sample count)")
        if isinstance(scale, bool) or not isinstance(scale, int) or not 1 <= scale <= SURFACE_SCALE_MAX:
            raise ValueError("shapeclipper_amd: render_surface takes an integer scale in 1..%d, got %r" % (SURFACE_SCALE_MAX, scale))
        if isinstance(n_refine, bool) or not isinstance(n_refine, int) or not 0 <= n_refine <= SURFACE_REFINE_MAX:
            raise ValueError("shapeclipper_amd: render_surface takes an integer n_refine in 0..%d, got %r" % (SURFACE_REFINE_MAX, n_refine))
        R = scale * scale * int(opt.H) * int(opt.W)
        if R % 16:
            raise ValueError("shapeclipper_amd: render_surface needs a multiple of 16 rays per image (the point layout of sdf_forward and "
                             "rgb_points_forward), got %d x %d" % (scale * int(opt.H), scale * int(opt.W)))
        return scale, n_refine, R

    @torch.no_grad()
    def render_surface(self, opt, pose, intr, scale_dist, proj_latent_sdf, proj_latent_rgb, n_refine=3, scale=1):
        """The sharp render of `--hip.surface_render`: every ray is shot at the solid {sdf < 0}, stops at the first place it enters it, and
        the colour and the unit normal are evaluated at that one point.  Inference only (no autograd, no random draws).

        pose [B,3,4], intr [B,3,3], scale_dist [B], latents [B,Z] as forward takes them.  scale = k in 1..4 renders k opt.H x k opt.W pixels
        of the same view (intrinsics diag(k, k, 1) intr, width k opt.W; at k = 1 the rays are those of the evaluation render bit for bit).
        -> SurfaceRender, R = k^2 opt.H opt.W rays per image in row-major pixel order:
             rgb    [B,R,3]  predicted colour where the ray hits, data.bgcolor where it misses
             mask   [B,R,1]  1 where hit != 0, else 0
             depth  [B,R,1]  t * depth_fac where it hits (t: distance along the unit ray), else 0
             normal [B,R,3]  unit SDF gradient at the surface point where it hits, else 0
             hit    [B,R]    int32: 1 a crossing was bracketed, 2 the ray starts inside the solid (the near sample stands in), 0 miss
        The chain: rays -> the S evaluation samples (linspace) -> value-only SDF at the R S points -> ops.ray_first_crossing -> n_refine
        rounds of (ops.ray_bracket_step, value-only SDF at its R points) -> a last ops.ray_bracket_step for the surface point ->
        SDF with gradient and feature and ops.rgb_points_forward at those R points.  Images go through it at most VIEWS_MAX_RAYS rays at a
        time; a ray does not depend on its batch neighbours.  NotImplementedError for eager architectures, unsupported sample counts and
        the orthographic camera (as render_views); ValueError for R % 16 != 0 and for scale / n_refine out of range."""
        k, n_refine, _ = self._surface_args(opt, n_refine, scale)
        packs = self.sdf_network.packed(proj_latent_sdf) + self.rgb_network.packed(proj_latent_rgb)
        return self._surface_chain(opt, pose, intr, scale_dist, packs, pose.shape[0], n_refine, k, VIEWS_MAX_RAYS)

    @torch.no_grad()
    def surface_depth_grey(self, opt, out, pose, intr, scale_dist, scale=1):
        """The grey picture of a SurfaceRender's depth, [B,R,1] in [0, 1]: the samples of a ray span t in [near, far] = camera.dist
        scale_dist -+ 0.7, i.e. depths [near, far] depth_fac of that pixel, and the picture is (depth - near depth_fac) / (1.4 depth_fac)
        clamped to [0, 1] -- 0 (black) at the near sample plane, 1 (white) at the far one -- and 1 where the ray misses."""
        k, _, R = self._surface_args(opt, 0, scale)
        intr = intr.contiguous().float()
        if k != 1:
            intr = intr * torch.tensor([float(k), float(k), 1.0], device=intr.device).view(1, 3, 1)
        depth_fac = CameraRaysFunction.apply(pose, intr, None, R, k * int(opt.W))[2].view(-1, R, 1)
        near = (float(opt.camera.dist) * scale_dist.float() - 0.7).view(-1, 1, 1)
        grey = ((out.depth - near * depth_fac) / (1.4 * depth_fac)).clamp(0, 1)
        return torch.where(out.hit.unsqueeze(-1) != 0, grey, torch.ones_like(grey))

    def _surface_chain(self, opt, pose, intr, scale_dist, packs, n_bias, n_refine, k, max_rays):
        """render_surface of N = pose.shape[0] images whose image i takes the per-image biases i % n_bias (render_views lays V views of B
        images out view-major), in passes of whole images and at most max_rays rays (one image at least)."""
        w_pack, cbias, v_pack, dbias = packs
        N, S, W = pose.shape[0], self.N_samples, k * int(opt.W)
        R = k * k * int(opt.H) * int(opt.W)
        sym = bool(self.sdf_network.force_symmetry)
        pose, intr = pose.contiguous().float(), intr.contiguous().float()
        if k != 1:      # diag(k, k, 1) @ intr: the first two rows times k, exact in fp32
            intr = intr * torch.tensor([float(k), float(k), 1.0], device=intr.device).view(1, 3, 1)
        dev = pose.device
        out = SurfaceRender(*(torch.empty(N, R, c, device=dev) for c in (3, 1, 1, 3)), torch.empty(N, R, device=dev, dtype=torch.int32))
        per = max(1, int(max_rays) // R)
        for i0 in range(0, N, per):
            n = min(per, N - i0)
            cb, db = cbias, dbias
            if (i0, n) != (0, n_bias):
                which = torch.arange(i0, i0 + n, device=dev) % n_bias
                cb, db = cbias.index_select(0, which), dbias.index_select(0, which)
            cam_loc, ray_dirs, depth_fac = CameraRaysFunction.apply(pose[i0:i0 + n], intr[i0:i0 + n], None, R, W)
            z_vals, points = RaySampleFunction.apply(cam_loc, ray_dirs, scale_dist[i0:i0 + n].contiguous().float(), None, R, float(opt.camera.dist), S)
            sdf = ops.sdf_forward(points, w_pack, cb, R * S, symmetric=sym, want_grad=False, want_feat=False)[0]
            del points
            br = ops.ray_first_crossing(z_vals, sdf, 0.0)
            del sdf, z_vals
            t, p = ops.ray_bracket_step(br, cam_loc, ray_dirs)
            for _ in range(n_refine):
                f = ops.sdf_forward(p, w_pack, cb, R, symmetric=sym, want_grad=False, want_feat=False)[0]
                t, p = ops.ray_bracket_step(br, cam_loc, ray_dirs, f, t)
            _, grad, feat = ops.sdf_forward(p, w_pack, cb, R, symmetric=sym, want_grad=True, want_feat=True)
            rgb, normal = ops.rgb_points_forward(p, grad, feat, v_pack, db, R, sym)
            hit = (br.hit != 0).unsqueeze(-1)
            sl = slice(i0, i0 + n)
            out.rgb[sl] = torch.where(hit, rgb, torch.full_like(rgb, self.bg_color)).view(n, R, 3)
            out.mask[sl] = hit.float().view(n, R, 1)
            out.depth[sl] = torch.where(hit, (t * depth_fac).unsqueeze(-1), torch.zeros_like(hit, dtype=torch.float32)).view(n, R, 1)
            out.normal[sl] = torch.where(hit, normal, torch.zeros_like(normal)).view(n, R, 3)
            out.hit[sl] = br.hit.view(n, R)
        return out

    def _forward_eager(self, opt, cam_loc, ray_dirs, depth_fac, scale_dist, t_rand, eik_idx, B, R, latent_sdf, latent_rgb, training, visualize,
                       up, rdev, pin):
        """The render on stock device operators (other architectures / sample counts): same random draws in the same order, same outputs."""
        from . import eager_path
        S = self.N_samples
        cam_loc, ray_dirs, depth_fac = cam_loc.reshape(-1, 3), ray_dirs.reshape(-1, 3), depth_fac.reshape(-1)
        centre = (opt.camera.dist * scale_dist).repeat_interleave(R).view(B * R, 1)
        t = torch.linspace(0.0, 1.0, steps=S, device=ray_dirs.device)
        z_vals = (centre - 0.7) * (1.0 - t) + (centre + 0.7) * t                      # reference renderer.py:17-24
        if training:
            mids = 0.5 * (z_vals[..., 1:] + z_vals[..., :-1])
            upper, lower = torch.cat([mids, z_vals[..., -1:]], -1), torch.cat([z_vals[..., :1], mids], -1)
            z_vals = lower + (upper - lower) * t_rand
        z_eik = torch.gather(z_vals, 1, eik_idx.unsqueeze(-1))
        eik = None
        if training:
            eik = up(torch.empty(B * R, 3, device=rdev, pin_memory=pin).uniform_(self.eik_range[0], self.eik_range[1])).reshape(B, R, 3)
        out = eager_path.render(self, opt, cam_loc, ray_dirs, depth_fac, z_vals, z_eik, eik, B, R, latent_sdf, latent_rgb, training)
        if not visualize:
            return out[:6]
        points_flat, alphas, rgb_flat = out[6]
        opacity = alphas.reshape(B, -1, 1)
        transp = torch.cat([opacity, 1 - opacity, torch.zeros_like(opacity)], dim=-1)
        rgba = torch.cat([rgb_flat.reshape(B, -1, 3), opacity], dim=-1)
        idx = torch.randperm(R)[:200].to(opacity.device)
        pick = lambda x: self.sample_rays_visualize(idx, x.reshape(B, R, S, -1))
        return out[:6] + (pick(points_flat.detach()), pick(transp), pick(rgba))

    def volume_rendering(self, z_vals, sdf):
        """Standalone torch form of reference renderer.py:187-209 for external callers (small tensors)."""
        density = self.density(sdf).reshape(-1, z_vals.shape[1])
        dists = torch.cat([z_vals[:, 1:] - z_vals[:, :-1], torch.zeros_like(z_vals[:, :1])], -1)
        free_energy = dists * density
        shifted = torch.cat([torch.zeros_like(free_energy[:, :1]), free_energy[:, :-1]], dim=-1)
        alpha = 1 - torch.exp(-free_energy)
        return alpha * torch.exp(-torch.cumsum(shifted, dim=-1)), alpha

    @torch.no_grad()
    def sample_rays_visualize(self, idx, item):
        item = item[:, idx].clone()
        return item.reshape(item.shape[0], -1, item.shape[-1])
