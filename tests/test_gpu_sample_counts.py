"""render.n_samples_uniform other than 64 on the HIP render kernels: any S with S % 32 == 0, 32 <= S <= 256 (csrc/render.hip,
rgb_fwd.hip, rgb_bwd.hip walk a ray in chunks of 64 samples).  Pinned against the float64 oracle (oracle/reference_ops.py renders any
S), against the torch formula of the sampler, against model/eager_path.py (what these sample counts ran on before) and against the
S = 64 entry points of the C ABI."""
import ctypes
import warnings
from contextlib import contextmanager

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SWITCHES = ("SDF_FWD_STREAM", "RGB_FWD_SPLIT", "RGB_BWD_SPLIT", "SDF_VALUE_SPLIT")
FLOOR = 2.0 ** -22
# the bars of tests/test_gpu_float64_budget.py
K_RENDER = dict(out=4.0, w_sdf=4.0, w_rgb=4.0, leaf=6.0, point_sum=16.0)
K_RGB = dict(out=4.0, point=8.0, w_rgb=4.0, latent=4.0)
POINT_SUMS = ("sdf_network.lin5.bias", "density.beta")


# ------------------------------------------------------------------------------------------------------------------------------------
# helpers (the float64-budget scheme of tests/test_gpu_float64_budget.py, with the sample count as a parameter)
# ------------------------------------------------------------------------------------------------------------------------------------
@contextmanager
def _switches(**kw):
    from shapeclipper_amd import ops
    saved = {k: getattr(ops, k) for k in kw}
    try:
        for k, v in kw.items():
            setattr(ops, k, v)
        yield
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)


def _twins():
    """The fp32-MFMA twins of the split kernels."""
    return _switches(**{k: False for k in SWITCHES})


def _err(x, x64):
    x64 = x64.detach().double().cpu()
    m = float(x64.abs().max())
    return float((x.detach().double().cpu() - x64).abs().max()) / m if m > 0 else float((x.detach().double().cpu()).abs().max())


def _check(title, rows, K, rule_a=True, floor=None):
    """rows: {name: (class, err default, err twins, err fp32 reference)}.  (a) default <= 1.5 twins + 2^-22 (not for point_sum: see
    test_training_render_float64_budget), (b) each arm <= K reference + floor (2^-22 unless floor[class] says otherwise)."""
    floor = floor or {}
    print("\n%s: max|X - X64| / max|X64|" % title)
    for n, (c, d, t, o) in rows.items():
        print("  %-28s %-9s %10.2e %10.2e %10.2e" % (n, c, d, t, o))
    bad_a = {n: (d, t) for n, (c, d, t, o) in rows.items() if c != "point_sum" and not d <= 1.5 * t + FLOOR}
    bad_b = {n: (c, d, t, o) for n, (c, d, t, o) in rows.items() if not max(d, t) <= K[c] * o + floor.get(c, FLOOR)}
    assert not (rule_a and bad_a), ("split arm worse than its fp32 twin", bad_a)
    assert not bad_b, ("HIP arm beyond K x the fp32 oracle", bad_b)


def _opt(H, W, S, extra=()):
    from shapeclipper_amd.utils import options
    o = options.set(options.parse_arguments(["--yaml=options/pix3d/config.yaml", "--name=pytest_ns", "--output_root=/tmp/sc_pytest",
                                             "--render.n_samples_uniform=%d" % S] + list(extra)), verbose=False)
    o.H, o.W = H, W
    return o


def _g12_weights(golden):
    g = golden("g12_render_hits")
    Ws = {k[len("w.sdf."):]: torch.tensor(g[k]) for k in g.files if k.startswith("w.sdf.")}
    Wr = {k[len("w.rgb."):]: torch.tensor(g[k]) for k in g.files if k.startswith("w.rgb.")}
    return Ws, Wr


def _cameras(cfg, B, seed):
    from oracle import reference_ops as R
    g = torch.Generator().manual_seed(seed)
    az = (torch.rand(B, generator=g) * 2 - 1) * np.pi
    el = (torch.rand(B, generator=g) - 0.5) * np.pi / 3
    trig = lambda t: torch.stack([torch.cos(t), torch.sin(t)], 1)
    sd = 0.9 + 0.2 * torch.rand(B, generator=g)
    pose = R.pose_from_trig(cfg, trig(az), trig(el), trig(torch.zeros(B)), sd)
    intr = R.get_intr(cfg, torch.ones(B))
    zs, zr = torch.randn(B, 64, generator=g) * 0.3, torch.randn(B, 64, generator=g) * 0.3
    return pose, intr, sd, zs, zr


def _fun(o, c):
    return ((o["rgb"] * c["rgb"]).sum() + (o["mask"] * c["mask"]).sum() + (o["depth"] * c["depth"]).sum()
            + (o["normal"] * c["normal"]).sum() + (o["eik"] * c["eik"]).sum())


def _oracle_render(cfg, Ws, Wr, beta, leaves, ray_idx, draws, cot, dt):
    from oracle import reference_ops as R
    t_rand, eik_idx, eik_pts = draws
    with R.default_dtype(dt):
        c = lambda t: t.detach().to(dt).clone().requires_grad_(True)
        oWs, oWr, ob = {k: c(v) for k, v in Ws.items()}, {k: c(v) for k, v in Wr.items()}, c(torch.tensor(beta))
        ol = {k: c(v) for k, v in leaves.items()}
        o = R.render(cfg, oWs, oWr, ob, ol["pose"], ol["intr"], ol["scale_dist"], ol["z_sdf"], ol["z_rgb"], ray_idx, True,
                     t_rand.to(dt), eik_idx, eik_pts.to(dt))
        o = dict(o, eik=o["grad_eikonal"])
        names = ["sdf_network." + k for k in oWs] + ["rgb_network." + k for k in oWr] + ["density.beta"] + list(ol)
        g = torch.autograd.grad(_fun(o, {k: v.to(dt) for k, v in cot.items()}),
                                list(oWs.values()) + list(oWr.values()) + [ob] + list(ol.values()), allow_unused=True)
    outs = {k: o[k].detach() for k in ("rgb", "mask", "mask_hard", "depth", "normal", "eik")}
    return outs, {n: (x if x is not None else torch.zeros_like(v)) for n, x, v in
                  zip(names, g, list(oWs.values()) + list(oWr.values()) + [ob] + list(ol.values()))}


def _renderer(opt, Ws, Wr, beta, eager=False):
    from shapeclipper_amd.model import eager_path
    from shapeclipper_amd.model.implicit import RGBNetwork, SDFNetwork
    from shapeclipper_amd.model.renderer import Renderer
    sdf_net, rgb_net = SDFNetwork(opt), RGBNetwork(opt)
    sdf_net.load_state_dict(Ws)
    rgb_net.load_state_dict(Wr)
    if eager:
        sdf_net.eager = rgb_net.eager = True
    eager_path._WARNED.clear()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = Renderer(opt, sdf_net, rgb_net).to(torch.device("cuda:0"))
    assert r.eager == eager
    assert eager or not any("stock PyTorch-ROCm operators" in str(x.message) for x in w)
    with torch.no_grad():
        r.density.beta.fill_(beta)
    return r


def _hip_render(opt, Ws, Wr, beta, leaves, ray_idx, cot, state, eager=False):
    dev = torch.device("cuda:0")
    r = _renderer(opt, Ws, Wr, beta, eager)
    lv = {k: v.detach().to(dev).requires_grad_(True) for k, v in leaves.items()}
    torch.set_rng_state(state)
    rgb, mask, mask_hard, depth, normal, eik = r(opt, lv["pose"], lv["intr"], lv["scale_dist"], lv["z_sdf"], lv["z_rgb"],
                                                 ray_idx=ray_idx.to(dev), training=True)
    o = dict(rgb=rgb, mask=mask, mask_hard=mask_hard, depth=depth, normal=normal, eik=eik)
    params = dict(r.named_parameters())
    names = list(params) + list(lv)
    g = torch.autograd.grad(_fun(o, {k: v.to(dev) for k, v in cot.items()}), [params[n] for n in params] + list(lv.values()), allow_unused=True)
    torch.cuda.synchronize()
    grads = {n: (x.cpu() if x is not None else torch.zeros_like(v).cpu()) for n, x, v in zip(names, g, list(params.values()) + list(lv.values()))}
    return {k: v.detach().cpu() for k, v in o.items()}, grads


def _render_rows(o64, g64, o32, g32, od, gd, ot, gt, ge=None):
    """ge: gradients of the eager path (model/eager_path.py, fp32 on the device); when given, a tensor's reference error is the larger of
    the fp32 oracle's and the eager path's."""
    hit = (o64["mask_hard"] > 0.5) & (o32["mask_hard"] > 0.5) & (od["mask_hard"] > 0.5) & (ot["mask_hard"] > 0.5)
    far = ((o64["mask"] - 0.5).abs() > 1e-3).expand_as(o64["normal"])
    rows = {}
    for k in ("rgb", "mask", "depth", "normal", "eik"):
        sel = (lambda x: x * (hit & far)) if k == "normal" else (lambda x: x)
        rows["out." + k] = ("out", _err(sel(od[k]), sel(o64[k])), _err(sel(ot[k]), sel(o64[k])), _err(sel(o32[k]), sel(o64[k])))
    for n in g64:
        if float(g64[n].abs().max()) == 0.0:
            continue
        c = "w_sdf" if n.startswith("sdf_network.") else ("w_rgb" if n.startswith("rgb_network.") else "leaf")
        c = "point_sum" if n in POINT_SUMS else c
        ref = _err(g32[n], g64[n]) if ge is None else max(_err(g32[n], g64[n]), _err(ge[n], g64[n]))
        rows[n.replace("_network", "")] = (c, _err(gd[n], g64[n]), _err(gt[n], g64[n]), ref)
    return rows


def _training_case(golden, S, beta, B=4, Rr=512, seed=7):
    """Leaves, rays, the CPU-generator state the renderer replays, the oracle's draws and cotangents (normals only where rays hit)."""
    from oracle import reference_ops as R
    cfg = R.Cfg(H=224, W=224, n_samples=S)
    Ws, Wr = _g12_weights(golden)
    pose, intr, sd, zs, zr = _cameras(cfg, B, seed=seed)
    leaves = dict(pose=pose, intr=intr, scale_dist=sd, z_sdf=zs, z_rgb=zr)
    gen = torch.Generator().manual_seed(8)
    ray_idx = torch.stack([torch.randperm(224 * 224, generator=gen)[:Rr] for _ in range(B)])
    torch.manual_seed(1234)
    state = torch.get_rng_state()
    draws = R.draw_render_randoms(B * Rr, S, True)
    cot = dict(rgb=torch.randn(B, Rr, 3, generator=gen), mask=torch.randn(B, Rr, 1, generator=gen),
               depth=torch.randn(B, Rr, 1, generator=gen), normal=torch.randn(B, Rr, 3, generator=gen),
               eik=torch.randn(2 * B * Rr, generator=gen))
    hit = R.render(cfg, Ws, Wr, torch.tensor(beta), pose, intr, sd, zs, zr, ray_idx, True, *draws)["mask_hard"].detach()
    cot["normal"] = cot["normal"] * hit
    return cfg, Ws, Wr, leaves, ray_idx, state, draws, cot


# ------------------------------------------------------------------------------------------------------------------------------------
# the Renderer takes the HIP path for the supported family, and only for it
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [32, 96, 128, 256])
def test_renderer_takes_the_hip_path_for_supported_sample_counts(golden, S):
    Ws, Wr = _g12_weights(golden)
    r = _renderer(_opt(8, 8, S), Ws, Wr, 0.05)          # asserts: not eager, no eager warning
    assert not r.eager and not r.sdf_network.eager and not r.rgb_network.eager


@pytest.mark.parametrize("S", [48, 320])
def test_other_sample_counts_stay_on_the_eager_path_and_say_so(golden, S):
    from shapeclipper_amd.model import eager_path
    from shapeclipper_amd.model.implicit import RGBNetwork, SDFNetwork
    from shapeclipper_amd.model.renderer import Renderer
    opt = _opt(8, 8, S)
    eager_path._WARNED.clear()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = Renderer(opt, SDFNetwork(opt), RGBNetwork(opt))
    assert r.eager
    assert any("render.n_samples_uniform = %d" % S in str(x.message) and "multiple of 32 from 32 to 256" in str(x.message) for x in w)


# ------------------------------------------------------------------------------------------------------------------------------------
# sampler: bit-identical to the torch formula, adjoint against autograd
# ------------------------------------------------------------------------------------------------------------------------------------
def _torch_sample(cam_loc, ray_dirs, scale_dist, u, R, dist, S):
    n = ray_dirs.shape[0]
    c = (dist * scale_dist).repeat_interleave(R).view(n, 1)
    near, far = c - 0.7, c + 0.7
    t = torch.linspace(0.0, 1.0, steps=S).to(ray_dirs.device)
    z = near * (1.0 - t) + far * t
    if u is not None:
        mids = 0.5 * (z[..., 1:] + z[..., :-1])
        upper = torch.cat([mids, z[..., -1:]], -1)
        lower = torch.cat([z[..., :1], mids], -1)
        z = lower + (upper - lower) * u
    pts = (cam_loc.unsqueeze(1) + z.unsqueeze(2) * ray_dirs.unsqueeze(1)).reshape(-1, 3)
    return z, pts


@pytest.mark.parametrize("eik", [False, True])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("S", [32, 96, 256])
def test_ray_sample_matches_torch_ops_and_adjoint(S, training, eik):
    from shapeclipper_amd.functional import RaySampleEikFunction, RaySampleFunction
    dev = torch.device("cuda:0")
    torch.manual_seed(S)
    B, R = 3, 37
    o = torch.randn(B * R, 3, device=dev, requires_grad=True)
    d = torch.nn.functional.normalize(torch.randn(B * R, 3, device=dev), dim=-1).requires_grad_(True)
    sd = (0.8 + 0.4 * torch.rand(B, device=dev)).requires_grad_(True)
    u = torch.rand(B * R, S, device=dev) if training else None
    zr, pr = _torch_sample(o, d, sd, u, R, 5.0, S)
    if eik:
        if not training:
            u = torch.zeros(B * R, S, device=dev)          # the eik launch is the training one; u = 0 is the lower bound of every stratum
            zr, pr = _torch_sample(o, d, sd, u, R, 5.0, S)
        idx = torch.randint(S, (B * R,), device=dev)
        idx[0], idx[1] = 0, S - 1                           # both ends of the ray, and the chunk edges
        if S > 64:
            idx[2], idx[3] = 63, 64
        eu = torch.rand(B * R, 3, device=dev)
        z, p, e = RaySampleEikFunction.apply(o, d, sd, u, idx, eu, R, 5.0)
        near = (o + torch.gather(zr, 1, idx.unsqueeze(1)) * d).view(B, R, 3)
        er = torch.cat([eu.view(B, R, 3), near], 1)
        assert torch.equal(e, er)
    else:
        z, p = RaySampleFunction.apply(o, d, sd, u, R, 5.0, S)
    assert z.shape == (B * R, S)
    assert torch.equal(z, zr), (z - zr).abs().max()
    assert torch.equal(p, pr)
    cz, cp = torch.randn_like(z), torch.randn_like(p)
    f = lambda zz, pp, ee: (zz * cz).sum() + (pp * cp).sum() + ((ee * ce).sum() if eik else 0.0)
    if eik:
        ce = torch.randn_like(e)
    g = torch.autograd.grad(f(z, p, e if eik else None), [o, d, sd])
    gr = torch.autograd.grad(f(zr, pr, er if eik else None), [o, d, sd])
    for a, b in zip(g, gr):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-4), (a - b).abs().max()


# ------------------------------------------------------------------------------------------------------------------------------------
# training render against float64: every output and every gradient, three arms
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.05, 0.005])
@pytest.mark.parametrize("S", [32, 128, 256])
def test_training_render_float64_budget(golden, S, beta):
    """Training render B=4 x R=512 at S samples per ray, G12 weights: outputs and every gradient, the bars of
    test_gpu_float64_budget.py with two findings of this shape.

    ReLU kinks (S = 32, beta 0.05): rgb lin0 / lin2 weight gradients are 5e-4 / 6e-4 of max off float64 in both HIP arms, 1.5e-4 /
    3e-5 for the fp32 oracle -- and exactly 5.13e-4 / 6.02e-4, worst rows 32, 43 / 47, 4, 9, for the eager path (stock device
    operators, what this sample count rendered on before).  A hidden pre-activation within fp32 rounding of zero switches its ReLU
    between fp32 evaluations of different operation order; which evaluation is lucky is a coin toss per unit (at S = 64 all three fp32
    arms sit at 1.06e-3 on rgb lin0).  So the fp32 reference of a tensor is the larger of the oracle's and the eager path's error.

    point_sum (sdf lin5 bias, beta): sums of one term per point in fp32 whose distance from float64 is set by the summation order (the
    finding of test_gpu_float64_budget.py); rule (a) does not apply to them, rule (b) with K = 16 does."""
    cfg, Ws, Wr, leaves, ray_idx, state, draws, cot = _training_case(golden, S, beta)
    opt = _opt(224, 224, S)
    o32, g32 = _oracle_render(cfg, Ws, Wr, beta, leaves, ray_idx, draws, cot, torch.float32)
    o64, g64 = _oracle_render(cfg, Ws, Wr, beta, leaves, ray_idx, draws, cot, torch.float64)
    od, gd = _hip_render(opt, Ws, Wr, beta, leaves, ray_idx, cot, state)
    with _twins():
        ot, gt = _hip_render(opt, Ws, Wr, beta, leaves, ray_idx, cot, state)
    _, ge = _hip_render(opt, Ws, Wr, beta, leaves, ray_idx, cot, state, eager=True)
    print("hit fraction %.2f" % float(o64["mask_hard"].mean()))
    _check("training render S=%d beta=%g; columns: default | twins | max(fp32 oracle, eager path)" % (S, beta),
           _render_rows(o64, g64, o32, g32, od, gd, ot, gt, ge), K_RENDER)


def test_eval_render_one_image_float64_budget(golden):
    """Evaluation render of one 64x64 image at S = 128 (524,288 points)."""
    from oracle import reference_ops as R
    S, beta, H = 128, 0.05, 64
    dev = torch.device("cuda:0")
    opt, cfg = _opt(H, H, S), R.Cfg(H=H, W=H, n_samples=S)
    Ws, Wr = _g12_weights(golden)
    pose, intr, sd, zs, zr = _cameras(cfg, 1, seed=11)

    def hip():
        r = _renderer(opt, Ws, Wr, beta)
        with torch.no_grad():
            o = r(opt, pose.to(dev), intr.to(dev), sd.to(dev), zs.to(dev), zr.to(dev), ray_idx=None, training=False)
        torch.cuda.synchronize()
        return dict(zip(("rgb", "mask", "mask_hard", "depth", "normal"), [x.cpu() for x in o[:5]]))
    od = hip()
    with _twins():
        ot = hip()
    ref = {}
    for dt in (torch.float32, torch.float64):
        _, eik_idx, _ = R.draw_render_randoms(H * H, S, False)
        with R.default_dtype(dt), torch.no_grad():
            c = lambda t: t.to(dt)
            o = R.render(cfg, {k: c(v) for k, v in Ws.items()}, {k: c(v) for k, v in Wr.items()}, torch.tensor(beta), c(pose), c(intr),
                         c(sd), c(zs), c(zr), torch.arange(H * H).view(1, -1), False, None, eik_idx, None)
        ref[dt] = {k: o[k] for k in ("rgb", "mask", "mask_hard", "depth", "normal")}
    o64, o32 = ref[torch.float64], ref[torch.float32]
    hit = (o64["mask_hard"] > 0.5) & (o32["mask_hard"] > 0.5) & (od["mask_hard"] > 0.5) & (ot["mask_hard"] > 0.5)
    hit = hit & ((o64["mask"] - 0.5).abs() > 1e-3)
    assert float(hit.float().mean()) > 0.05
    rows = {}
    for k in ("rgb", "mask", "depth", "normal"):
        sel = (lambda x: x * hit) if k == "normal" else (lambda x: x)
        rows["out." + k] = ("out", _err(sel(od[k]), sel(o64[k])), _err(sel(ot[k]), sel(o64[k])), _err(sel(o32[k]), sel(o64[k])))
    _check("evaluation render 64x64 S=%d" % S, rows, K_RENDER)


# ------------------------------------------------------------------------------------------------------------------------------------
# kernel level: rgb_composite forward + the four reverse variants and the > 256-image fallback
# ------------------------------------------------------------------------------------------------------------------------------------
def _rgb_case(n_images, rpi, S, seed):
    from oracle import reference_ops as R
    from shapeclipper_amd import ops, packing
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(seed)
    cfg = R.Cfg(n_samples=S)
    Ws, Wr = R.init_sdf_weights(cfg, 1), R.init_rgb_weights(cfg, 2)
    zs, zr = torch.randn(n_images, 64, generator=g) * 0.3, torch.randn(n_images, 64, generator=g) * 0.3
    n_rays = n_images * rpi
    pts = torch.rand(n_rays * S, 3, generator=g) * 1.6 - 0.8
    z = torch.sort(torch.rand(n_rays, S, generator=g) * 2 + 4, dim=1).values
    dfac = torch.rand(n_rays, generator=g) * 0.2 + 0.9
    sdf_pack, cb = packing.pack_sdf({k: v.to(dev) for k, v in Ws.items()}, zs.to(dev))
    sdf, grad, feat = ops.sdf_forward(pts.to(dev), sdf_pack, cb, rpi * S)
    # a thin shell of density along the whole ray (sdf ~ beta): every chunk carries weight, so the carries of E and of the suffix sums
    # across chunk edges are exercised
    ins = dict(points=pts, z_vals=z, depth_fac=dfac, sdf=(sdf.cpu() * 0.05 + 0.12), grad=grad.cpu(),
               feat=packing.tbl_to_rows(feat, n_rays * S).cpu(), beta=torch.tensor([0.1]))
    return cfg, ins, Wr, zr


def _rgb_oracle(cfg, ins, Wr, zr, rpi, cot, dt):
    import torch.nn.functional as F
    from oracle import reference_ops as R
    S = cfg.n_samples
    with R.default_dtype(dt):
        L = {k: v.to(dt).clone().requires_grad_(True) for k, v in ins.items()}
        Wl = {k: v.to(dt).clone().requires_grad_(True) for k, v in Wr.items()}
        zl = zr.to(dt).clone().requires_grad_(True)
        rgb_flat = R.rgb_mlp(cfg, Wl, L["points"], zl.repeat_interleave(rpi * S, 0), L["feat"])
        s = L["sdf"].view(-1, 1)
        dens = R.laplace_density(s, L["beta"], cfg.beta_min)
        normal_flat = -torch.autograd.grad(dens.sum(), s, create_graph=True)[0] * L["grad"]
        w, _ = R.volume_rendering(L["z_vals"], s, L["beta"], cfg.beta_min)
        acc = w.sum(-1)
        o = dict(rgb=(w.unsqueeze(-1) * rgb_flat.view(-1, S, 3)).sum(1) + (1.0 - acc.unsqueeze(1)) * cfg.bgcolor, mask=acc,
                 depth=(w * (L["z_vals"] * L["depth_fac"].unsqueeze(1))).sum(1),
                 normal=F.normalize((w.unsqueeze(-1) * F.normalize(normal_flat, dim=-1).view(-1, S, 3)).sum(1), dim=-1))
        outs = {k: v.detach() for k, v in o.items()}
        outs["mask_hard"] = (acc > 0.5).to(acc.dtype).detach()
        if cot is None:
            return outs, None
        f = sum((o[k] * cot[k].to(dt)).sum() for k in cot)
        names = list(L) + ["rgb_network." + k for k in Wl] + ["z_rgb"]
        gs = torch.autograd.grad(f, list(L.values()) + list(Wl.values()) + [zl])
    return outs, dict(zip(names, [x.detach() for x in gs]))


def _rgb_hip(ins, Wr, zr, rpi, cot):
    from shapeclipper_amd import packing
    from shapeclipper_amd.functional import RgbCompositeFunction
    dev = torch.device("cuda:0")
    n_pts = ins["points"].shape[0]
    L = {k: (packing.rows_to_tbl(v) if k == "feat" else v).to(dev).contiguous().requires_grad_(True) for k, v in ins.items()}
    Wd = {k: v.to(dev).requires_grad_(True) for k, v in Wr.items()}
    zd = zr.to(dev).requires_grad_(True)
    v_pack, dbias = packing.pack_rgb(Wd, zd)
    rgb, mask, mask_hard, depth, normal = RgbCompositeFunction.apply(L["points"], L["z_vals"], L["depth_fac"], L["sdf"], L["grad"], L["feat"],
                                                                     v_pack, dbias, L["beta"], rpi, True, 1e-4, 1.0, 1.0, False)
    o = dict(rgb=rgb, mask=mask, depth=depth, normal=normal)
    f = sum((o[k] * cot[k].to(dev)).sum() for k in cot)
    names = list(L) + ["rgb_network." + k for k in Wd] + ["z_rgb"]
    gs = torch.autograd.grad(f, list(L.values()) + list(Wd.values()) + [zd])
    torch.cuda.synchronize()
    grads = {n: x.cpu() for n, x in zip(names, gs)}
    grads["feat"] = packing.tbl_to_rows(gs[list(L).index("feat")], n_pts).cpu()
    outs = {k: v.detach().cpu() for k, v in o.items()}
    outs["mask_hard"] = mask_hard.cpu()
    return outs, grads


def _rgb_refs(n_images, rpi, S):
    cfg, ins, Wr, zr = _rgb_case(n_images, rpi, S, seed=n_images * 100 + rpi + S)
    n_rays = n_images * rpi
    o64, _ = _rgb_oracle(cfg, ins, Wr, zr, rpi, None, torch.float64)
    hit = ((o64["mask"] - 0.5).abs() > 1e-3) & (o64["mask"] > 0.5)
    g = torch.Generator().manual_seed(rpi)
    cot = dict(rgb=torch.randn(n_rays, 3, generator=g), mask=torch.randn(n_rays, generator=g), depth=torch.randn(n_rays, generator=g),
               normal=torch.randn(n_rays, 3, generator=g) * hit.unsqueeze(1))
    o64, g64 = _rgb_oracle(cfg, ins, Wr, zr, rpi, cot, torch.float64)
    o32, g32 = _rgb_oracle(cfg, ins, Wr, zr, rpi, cot, torch.float32)
    return (ins, Wr, zr, hit, cot), (o64, g64, o32, g32)


def _rgb_rows(ref, hit, od, gd, ot, gt):
    o64, g64, o32, g32 = ref
    rows = {}
    for k in ("rgb", "mask", "depth", "normal"):
        sel = (lambda x: x * hit.unsqueeze(1)) if k == "normal" else (lambda x: x)
        rows["out." + k] = ("out", _err(sel(od[k]), sel(o64[k])), _err(sel(ot[k]), sel(o64[k])), _err(sel(o32[k]), sel(o64[k])))
    for n in g64:
        if float(g64[n].abs().max()) == 0.0:
            continue
        c = "w_rgb" if n.startswith("rgb_network.") else ("latent" if n == "z_rgb" else "point")
        rows[n] = (c, _err(gd[n], g64[n]), _err(gt[n], g64[n]), _err(g32[n], g64[n]))
    return rows


# variant: (switches of the arm compared with the default, rule (a) applies)
RGB_VARIANTS = {"split_vs_twins": (dict(RGB_FWD_SPLIT=False, RGB_BWD_SPLIT=False), True),          # _fused_split | _fused_stash
                "recompute": (dict(RGB_STASH=False), False),                                       # _fused (no parked activations)
                "v3_wgrad": (dict(FUSED_RGB_WGRAD=False), False)}                                 # _v3 + three sc_wgrad launches


# The reverse forms that read the parked activations evaluate the encoding's Jacobian with the hardware sine / cosine (rgb_bwd.hip, pe_slots
# FAST): measured on these inputs, the point gradient of that arm is 1.47e-6 of max off float64 at S = 64 (1.60e-6 at S = 32) while the
# fp32 oracle's error moves between 1.3e-7 and 3.6e-7 -- a floor of the S = 64 kernels, not of the sample count.
RGB_FLOOR = dict(point=2.0 ** -18)


@pytest.mark.parametrize("variant", list(RGB_VARIANTS))
@pytest.mark.parametrize("S", [32, 128])
def test_rgb_composite_float64_budget(S, variant):
    kw, rule_a = RGB_VARIANTS[variant]
    n_images, rpi = 3, 37
    (ins, Wr, zr, hit, cot), ref = _rgb_refs(n_images, rpi, S)
    od, gd = _rgb_hip(ins, Wr, zr, rpi, cot)
    with _switches(**kw):
        ot, gt = _rgb_hip(ins, Wr, zr, rpi, cot)
    assert torch.equal(od["mask_hard"], ot["mask_hard"])
    print("hit fraction %.2f" % float(hit.float().mean()))
    _check("RGB composite S=%d; columns: default | %s | fp32 oracle" % (S, variant), _rgb_rows(ref, hit, od, gd, ot, gt), K_RGB, rule_a=rule_a,
           floor=RGB_FLOOR)


@pytest.mark.parametrize("S", [32, 128])
def test_rgb_composite_257_images_float64_budget(S):
    """257 images: past the 256-image limit of the fused backward, the default takes _v3 + sc_wgrad."""
    n_images, rpi = 257, 4
    (ins, Wr, zr, hit, cot), ref = _rgb_refs(n_images, rpi, S)
    od, gd = _rgb_hip(ins, Wr, zr, rpi, cot)
    with _twins():
        ot, gt = _rgb_hip(ins, Wr, zr, rpi, cot)
    _check("RGB composite n_images=257 S=%d" % S, _rgb_rows(ref, hit, od, gd, ot, gt), K_RGB, rule_a=False, floor=RGB_FLOOR)


# ------------------------------------------------------------------------------------------------------------------------------------
# HIP against model/eager_path.py (what S != 64 ran on before) with the same draws; determinism
# ------------------------------------------------------------------------------------------------------------------------------------
def test_hip_matches_the_eager_path_at_96_samples(golden):
    S, beta = 96, 0.05
    cfg, Ws, Wr, leaves, ray_idx, state, draws, cot = _training_case(golden, S, beta, B=2, Rr=256)
    opt = _opt(224, 224, S)
    oh, gh = _hip_render(opt, Ws, Wr, beta, leaves, ray_idx, cot, state)
    oe, ge = _hip_render(opt, Ws, Wr, beta, leaves, ray_idx, cot, state, eager=True)
    guard = (oe["mask"] - 0.5).abs() > 1e-5
    assert torch.equal(oh["mask_hard"][guard], oe["mask_hard"][guard])
    for k in ("rgb", "mask", "depth", "normal", "eik"):
        tol = 2e-4 if k in ("normal", "eik", "depth") else 2e-5                  # the bars of tests/test_gpu_parity_large.py
        want = oe[k] * (oe["mask_hard"] > 0.5) if k == "normal" else oe[k]
        got = oh[k] * (oe["mask_hard"] > 0.5) if k == "normal" else oh[k]
        assert (got - want).abs().max() < tol * max(1.0, float(want.abs().max())), (k, float((got - want).abs().max()))
    worst = {n: float((gh[n] - ge[n]).abs().max()) / max(float(ge[n].abs().max()), 1e-4) for n in ge}
    bad = {k: v for k, v in worst.items() if v > (1e-3 if k in ("pose", "intr", "scale_dist") else 2e-4)}
    print("HIP vs eager at S=96: worst gradient error %.1e" % max(worst.values()))
    assert not bad, bad


def test_training_render_is_deterministic_at_128_samples(golden):
    S, beta = 128, 0.05
    cfg, Ws, Wr, leaves, ray_idx, state, draws, cot = _training_case(golden, S, beta, B=2, Rr=512)
    opt = _opt(224, 224, S)
    o1, g1 = _hip_render(opt, Ws, Wr, beta, leaves, ray_idx, cot, state)
    o2, g2 = _hip_render(opt, Ws, Wr, beta, leaves, ray_idx, cot, state)
    for k in o1:
        assert torch.equal(o1[k], o2[k]), k
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n


# ------------------------------------------------------------------------------------------------------------------------------------
# C ABI: the _ns entry points at S = 64 are the old symbols; S outside the family is refused
# ------------------------------------------------------------------------------------------------------------------------------------
def _abi_inputs(n_images=2, rpi=20, S=64):
    cfg, ins, Wr, zr = _rgb_case(n_images, rpi, S, seed=5)
    from shapeclipper_amd import packing
    dev = torch.device("cuda:0")
    d = {k: (packing.rows_to_tbl(v) if k == "feat" else v).to(dev).contiguous() for k, v in ins.items()}
    v_pack, dbias = packing.pack_rgb({k: v.to(dev) for k, v in Wr.items()}, zr.to(dev))
    return d, v_pack.contiguous(), dbias.contiguous(), n_images * rpi, rpi, n_images


def test_ns_entry_points_at_64_samples_equal_the_old_symbols_and_refuse_other_counts():
    from shapeclipper_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    d, v_pack, dbias, n_rays, rpi, n_img = _abi_inputs()
    P, T = n_rays * 64, n_rays * 4 * 1024
    E = lambda *s: torch.full(s, float("nan"), device=dev)
    p, f, i = _lib.ptr, ctypes.c_float, ctypes.c_int
    head = lambda: (p(d["points"]), p(d["z_vals"]), p(d["depth_fac"]), p(d["sdf"]), p(d["grad"]), p(d["feat"]), p(v_pack), p(dbias),
                    p(d["beta"]))
    tail = (i(rpi), i(n_img), i(1), f(1e-4), f(1.0), f(1.0))

    def fwd(name, ns, rr):
        o = dict(rgb=E(n_rays, 3), mask=E(n_rays), mh=E(n_rays), depth=E(n_rays), normal=E(n_rays, 3), w=E(n_rays, 64), a=E(n_rays, 64),
                 flat=E(P, 3), rr=E(3 * T))
        args = head() + (i(n_rays),) + ((i(ns),) if ns is not None else ()) + tail + tuple(p(o[k]) for k in ("rgb", "mask", "mh", "depth", "normal", "w", "a", "flat"))
        args += ((p(o["rr"]),) if rr else ()) + (_lib.stream(),)
        rc = getattr(lib, name)(*args)
        torch.cuda.synchronize()
        return rc, o
    for base, rr in (("sc_rgb_composite_forward", False), ("sc_rgb_composite_forward_stash", True), ("sc_rgb_composite_forward_split", True)):
        rc0, o0 = fwd(base, None, rr)
        rc1, o1 = fwd(base + "_ns", 64, rr)
        assert rc0 == 0 and rc1 == 0
        for k in o0:
            if k != "rr" or rr:
                assert torch.equal(o0[k].nan_to_num(7.0), o1[k].nan_to_num(7.0)), (base, k)
        for bad in (48, 0, 288):
            assert fwd(base + "_ns", bad, rr)[0] == 1, (base, bad)           # hipErrorInvalidValue

    _, ofw = fwd("sc_rgb_composite_forward_stash", None, True)
    G = dict(rgb=torch.randn(n_rays, 3, device=dev), mask=torch.randn(n_rays, device=dev), depth=torch.randn(n_rays, device=dev),
             normal=torch.randn(n_rays, 3, device=dev))

    def bwd(name, ns, kind):
        parts = int(lib.sc_rgb_composite_backward_fused_parts(i(n_rays)))
        stride = int(lib.sc_rgb_composite_backward_fused_partial_floats(i(n_img)))
        o = dict(sdf=E(P), grad=E(P, 3), feat=E(T), pts=E(P, 3), z=E(n_rays, 64), dfac=E(n_rays), beta=E(2048), v3=E(2048 * 196),
                 part=E(parts * stride), gy=E(3 * T), rr=E(2 * T))
        args = head() + (p(ofw["flat"]), i(n_rays)) + ((i(ns),) if ns is not None else ()) + tail
        args += (p(G["rgb"]), p(G["mask"]), p(G["depth"]), p(G["normal"])) + tuple(p(o[k]) for k in ("sdf", "grad", "feat", "pts", "z", "dfac", "beta"))
        if kind == "v3":
            args += (p(o["gy"]), p(o["rr"]), None, p(o["v3"]))
        else:
            args += (p(o["part"]), p(o["v3"])) + ((p(ofw["rr"]),) if kind == "rr" else ())
        rc = getattr(lib, name)(*(args + (_lib.stream(),)))
        torch.cuda.synchronize()
        return rc, o
    for base, kind in (("sc_rgb_composite_backward_v3", "v3"), ("sc_rgb_composite_backward_fused", "plain"),
                       ("sc_rgb_composite_backward_fused_stash", "rr"), ("sc_rgb_composite_backward_fused_split", "rr")):
        rc0, o0 = bwd(base, None, kind)
        rc1, o1 = bwd(base + "_ns", 64, kind)
        assert rc0 == 0 and rc1 == 0
        for k in o0:
            assert torch.equal(o0[k].nan_to_num(7.0), o1[k].nan_to_num(7.0)), (base, k)
        for bad in (48, 0, 288):
            assert bwd(base + "_ns", bad, kind)[0] == 1, (base, bad)

    # the sampler pair
    o = torch.randn(n_rays, 3, device=dev)
    dd = torch.nn.functional.normalize(torch.randn(n_rays, 3, device=dev), dim=-1)
    sd = 0.8 + 0.4 * torch.rand(n_img, device=dev)
    u = torch.rand(n_rays, 64, device=dev)
    idx = torch.randint(64, (n_rays,), device=dev)
    eu = torch.rand(n_rays, 3, device=dev)

    def samp(name, ns):
        z, pts, e = E(n_rays, 64), E(P, 3), E(n_img, 2 * rpi, 3)
        if "eik" in name:
            args = (p(o), p(dd), p(sd), p(u), p(idx), p(eu), i(n_rays)) + ((i(ns),) if ns is not None else ()) + (i(rpi), i(n_img), f(5.0), p(z), p(pts), p(e))
        else:
            args = (p(o), p(dd), p(sd), p(u), i(n_rays)) + ((i(ns),) if ns is not None else ()) + (i(rpi), i(n_img), f(5.0), p(z), p(pts))
        rc = getattr(lib, name)(*(args + (_lib.stream(),)))
        torch.cuda.synchronize()
        return rc, (z, pts, e)
    gp, gz, ge = torch.randn(P, 3, device=dev), torch.randn(n_rays, 64, device=dev), torch.randn(n_img, 2 * rpi, 3, device=dev)

    def samp_b(name, ns):
        go, gd, gs = E(n_rays, 3), E(n_rays, 3), E(n_rays)
        zv = samp("sc_ray_sample_forward", None)[1][0]
        if "eik" in name:
            args = (p(dd), p(zv), p(gp), p(gz), p(idx), p(ge), i(n_rays)) + ((i(ns),) if ns is not None else ()) + (i(rpi), i(n_img), f(5.0))
        else:
            args = (p(dd), p(zv), p(gp), p(gz), i(n_rays)) + ((i(ns),) if ns is not None else ()) + (i(rpi), i(n_img), f(5.0))
        rc = getattr(lib, name)(*(args + (p(go), p(gd), p(gs), _lib.stream())))
        torch.cuda.synchronize()
        return rc, (go, gd, gs)
    for fn, base in ((samp, "sc_ray_sample_forward"), (samp, "sc_ray_sample_forward_eik"), (samp_b, "sc_ray_sample_backward"),
                     (samp_b, "sc_ray_sample_backward_eik")):
        rc0, a0 = fn(base, None)
        rc1, a1 = fn(base + "_ns", 64)
        assert rc0 == 0 and rc1 == 0
        for x, y in zip(a0, a1):
            assert torch.equal(x.nan_to_num(7.0), y.nan_to_num(7.0)), base
        for bad in (48, 0, 288):
            assert fn(base + "_ns", bad)[0] == 1, (base, bad)


# ------------------------------------------------------------------------------------------------------------------------------------
# one training step through model/graph.py at 32 samples per ray
# ------------------------------------------------------------------------------------------------------------------------------------
def test_training_step_at_32_samples_runs_on_the_hip_path():
    import os
    import time
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    from shapeclipper_amd import synthetic
    from shapeclipper_amd.model import eager_path
    from shapeclipper_amd.model.runner import Runner
    from shapeclipper_amd.utils import options, util
    from shapeclipper_amd.utils.util import EasyDict as edict
    opt = options.set(options.parse_arguments(["--yaml=options/pix3d/config.yaml", "--name=pytest_step_ns", "--output_root=/tmp/sc_pytest",
                                               "--batch_size=4", "--tb!", "--arch.enc_pretrained!", "--render.n_samples_uniform=32"]),
                      verbose=False)
    opt.device, opt.world_size, opt.port = 0, 1, 0
    opt.freq.scalar, opt.freq.ckpt_latest = 0, 10 ** 9
    torch.manual_seed(0)
    eager_path._WARNED.clear()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        runner = Runner(opt)
        runner.build_networks(opt)
        runner.setup_optimizer(opt)
        runner.graph.train()
        runner.it, runner.ep, runner.best_val = 1, 0, 0.0
        runner.timer = edict(start=time.time(), it_mean=None)
        batch = util.move_to_device(synthetic.make_batch(opt, 4, seed=0), "cuda:0")
        opt.H, opt.W = opt.image_size
        loss = runner.train_iteration(opt, edict(batch), None)
    assert not any("stock PyTorch-ROCm operators" in str(x.message) for x in w)
    g = runner.graph.module
    assert g.renderer.N_samples == 32 and not g.renderer.eager
    assert all(torch.isfinite(torch.as_tensor(float(v))) for v in loss.values()), loss
