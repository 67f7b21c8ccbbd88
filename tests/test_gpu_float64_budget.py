"""Float64 error budgets of the render chain.

The bf16x3 "split" kernels (exact three-piece bf16 splits, six of the nine piece products accumulated in fp32) are accepted as
fp32-equivalent on one condition: against float64 their error is no larger than that of their fp32-MFMA twins.  The fp32 oracle is
itself ~1e-5 .. 1e-4 of max away from exact arithmetic on these quantities, so comparing with it cannot tell a kernel's rounding from
the oracle's: a kernel that dropped a bf16 piece (2^-17 relative per weight) would pass.  Here every tensor is compared with the
oracle evaluated in float64 (oracle/reference_ops.py under R.default_dtype(torch.float64)), err(X) = max|X - X64| / max|X64|, in
three arms: the HIP default (every split switch on), the HIP fp32 twins (ops.SDF_FWD_STREAM / RGB_FWD_SPLIT / RGB_BWD_SPLIT /
SDF_VALUE_SPLIT off) and the fp32 oracle.  Per tensor:

  (a) err(default) <= 1.5 err(twins) + 2^-22                     the ruling's own condition
  (b) err(each HIP arm) <= K err(fp32 oracle) + 2^-22             K per tensor class, below

Every test prints its three-arm table."""
from contextlib import contextmanager

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SWITCHES = ("SDF_FWD_STREAM", "RGB_FWD_SPLIT", "RGB_BWD_SPLIT", "SDF_VALUE_SPLIT")
FLOOR = 2.0 ** -22


@contextmanager
def _twins():
    """The fp32-MFMA twins of the split kernels; the switches are restored however the block exits."""
    from shapeclipper_amd import ops
    saved = {k: getattr(ops, k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            setattr(ops, k, False)
        yield
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)


def _err(x, x64):
    x64 = x64.detach().double().cpu()
    m = float(x64.abs().max())
    return float((x.detach().double().cpu() - x64).abs().max()) / m if m > 0 else float((x.detach().double().cpu()).abs().max())


def _check(title, rows, K, rule_a=True):
    """rows: {name: (class, err default, err twins, err fp32 oracle)}; K: {class: factor}.  Prints the table, then asserts (a) (unless the
    two HIP arms run the same kernel) and (b)."""
    print("\n%s: max|X - X64| / max|X64|" % title)
    print("  %-28s %-8s %10s %10s %10s %8s %8s" % ("tensor", "class", "default", "twins", "oracle32", "def/orc", "twin/orc"))
    for n, (c, d, t, o) in rows.items():
        print("  %-28s %-8s %10.2e %10.2e %10.2e %8.2f %8.2f" % (n, c, d, t, o, d / max(o, 1e-30), t / max(o, 1e-30)))
    bad_a = {n: (d, t) for n, (c, d, t, o) in rows.items() if not d <= 1.5 * t + FLOOR}
    bad_b = {n: (c, d, t, o) for n, (c, d, t, o) in rows.items() if not max(d, t) <= K[c] * o + FLOOR}
    assert not (rule_a and bad_a), ("split arm worse than its fp32 twin", bad_a)
    assert not bad_b, ("HIP arm beyond K x the fp32 oracle", bad_b)


# ---------------------------------------------------------------------------------------------------------------------------------
# kernel: ops.sdf_forward, training form (sdf, d sdf/dx, feature)
# ---------------------------------------------------------------------------------------------------------------------------------
K_SDF = dict(sdf=4.0, grad=4.0, feat=4.0)          # measured: <= 1.8 (sdf), 2.5 (grad), 1.8 (feat) x the fp32 oracle


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("B,N", [(1, 1), (2, 17), (3, 1371), (1, 40000)])
def test_sdf_forward_float64_budget(B, N, symmetric):
    """sc_sdf_forward_stream (default) / sc_sdf_forward (twin) against R.sdf_conditional in float64.  A one-point call is repeated
    for 32 points (32 launches): the error of ONE rounded value says nothing about an arm (measured at N=1: default 3.3e-7, twin
    2.6e-10 on one point)."""
    from oracle import reference_ops as R
    from shapeclipper_amd import ops, packing
    cfg = R.Cfg(force_symmetry=symmetric)
    g = torch.Generator().manual_seed(B * 1000 + N)
    W = {k: v + 0.05 * torch.randn(v.shape, generator=g) for k, v in R.init_sdf_weights(cfg, 1).items()}
    z = torch.randn(B, 64, generator=g)
    reps = 32 if B * N < 16 else 1
    pts = torch.rand(reps * B * N, 3, generator=g) * 2 - 1
    ref = {}
    for dt in (torch.float32, torch.float64):
        with R.default_dtype(dt):
            parts = [R.sdf_conditional(cfg, {k: v.to(dt) for k, v in W.items()}, B, p.to(dt).clone(), z.to(dt), compute_grad=True)
                     for p in pts.split(B * N)]
        ref[dt] = dict(sdf=torch.cat([s[:, 0].detach() for s, _, _ in parts]), grad=torch.cat([gr.detach() for _, _, gr in parts]),
                       feat=torch.cat([f.detach() for _, f, _ in parts]))
    dev = torch.device("cuda:0")
    pack, cb = packing.pack_sdf({k: v.to(dev) for k, v in W.items()}, z.to(dev))

    def hip():
        outs = [ops.sdf_forward(p.to(dev), pack, cb, N, symmetric=symmetric, want_grad=True, want_feat=True) for p in pts.split(B * N)]
        return dict(sdf=torch.cat([s for s, _, _ in outs]), grad=torch.cat([gr for _, gr, _ in outs]),
                    feat=torch.cat([packing.tbl_to_rows(f, B * N) for _, _, f in outs]))
    d = hip()
    with _twins():
        t = hip()
    torch.cuda.synchronize()
    rows = {k: (k, _err(d[k], ref[torch.float64][k]), _err(t[k], ref[torch.float64][k]), _err(ref[torch.float32][k], ref[torch.float64][k]))
            for k in ("sdf", "grad", "feat")}
    _check("sdf_forward B=%d N=%d symmetric=%s" % (B, N, symmetric), rows, K_SDF)


# ---------------------------------------------------------------------------------------------------------------------------------
# module: training render at the G12 shape (B=4 x R=512, rays that hit), outputs and every gradient, plus stress variants
# ---------------------------------------------------------------------------------------------------------------------------------
# measured over the five variants: out <= 1.1, w_sdf <= 1.8, w_rgb <= 2.2, leaf <= 3.4 x the fp32 oracle; point_sum <= 12.6 (see the test)
K_RENDER = dict(out=4.0, w_sdf=4.0, w_rgb=4.0, leaf=6.0, point_sum=16.0)
POINT_SUMS = ("sdf_network.lin5.bias", "density.beta")


def _opt(H, W):
    from shapeclipper_amd.utils import options
    o = options.set(options.parse_arguments(["--yaml=options/pix3d/config.yaml", "--name=pytest", "--output_root=/tmp/sc_pytest"]),
                    verbose=False)
    o.H, o.W = H, W
    return o


def _g12_weights(golden):
    g = golden("g12_render_hits")
    Ws = {k[len("w.sdf."):]: torch.tensor(g[k]) for k in g.files if k.startswith("w.sdf.")}
    Wr = {k[len("w.rgb."):]: torch.tensor(g[k]) for k in g.files if k.startswith("w.rgb.")}
    return Ws, Wr


def _cameras(cfg, B, seed, sd=None):
    from oracle import reference_ops as R
    g = torch.Generator().manual_seed(seed)
    az = (torch.rand(B, generator=g) * 2 - 1) * np.pi
    el = (torch.rand(B, generator=g) - 0.5) * np.pi / 3
    trig = lambda t: torch.stack([torch.cos(t), torch.sin(t)], 1)
    sd_draw = 0.9 + 0.2 * torch.rand(B, generator=g)
    sd = sd_draw if sd is None else torch.full((B,), float(sd))
    pose = R.pose_from_trig(cfg, trig(az), trig(el), trig(torch.zeros(B)), sd)
    intr = R.get_intr(cfg, torch.ones(B))
    zs, zr = torch.randn(B, 64, generator=g) * 0.3, torch.randn(B, 64, generator=g) * 0.3
    return pose, intr, sd, zs, zr


def _fun(o, c):
    return ((o["rgb"] * c["rgb"]).sum() + (o["mask"] * c["mask"]).sum() + (o["depth"] * c["depth"]).sum()
            + (o["normal"] * c["normal"]).sum() + (o["eik"] * c["eik"]).sum())


def _oracle_render(cfg, Ws, Wr, beta, leaves, ray_idx, draws, cot, dt):
    """The oracle's training render in dtype dt: outputs and the gradients of the cotangent functional, by name."""
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


def _hip_render(opt, Ws, Wr, beta, leaves, ray_idx, cot, state):
    from shapeclipper_amd.model.implicit import RGBNetwork, SDFNetwork
    from shapeclipper_amd.model.renderer import Renderer
    dev = torch.device("cuda:0")
    sdf_net, rgb_net = SDFNetwork(opt), RGBNetwork(opt)
    sdf_net.load_state_dict(Ws)
    rgb_net.load_state_dict(Wr)
    r = Renderer(opt, sdf_net, rgb_net).to(dev)
    with torch.no_grad():
        r.density.beta.fill_(beta)
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


def _render_rows(o64, g64, o32, g32, od, gd, ot, gt):
    hit = (o64["mask_hard"] > 0.5) & (o32["mask_hard"] > 0.5) & (od["mask_hard"] > 0.5) & (ot["mask_hard"] > 0.5)
    far = ((o64["mask"] - 0.5).abs() > 1e-3).expand_as(o64["normal"])
    rows = {}
    for k in ("rgb", "mask", "depth", "normal", "eik"):
        sel = (lambda x: x * (hit & far)) if k == "normal" else (lambda x: x)      # normals of rays that miss: rounding noise in any precision
        rows["out." + k] = ("out", _err(sel(od[k]), sel(o64[k])), _err(sel(ot[k]), sel(o64[k])), _err(sel(o32[k]), sel(o64[k])))
    for n in g64:
        if float(g64[n].abs().max()) == 0.0:
            continue
        c = "w_sdf" if n.startswith("sdf_network.") else ("w_rgb" if n.startswith("rgb_network.") else "leaf")
        c = "point_sum" if n in POINT_SUMS else c
        rows[n.replace("_network", "")] = (c, _err(gd[n], g64[n]), _err(gt[n], g64[n]), _err(g32[n], g64[n]))
    return rows


VARIANTS = {
    "g12": dict(beta=0.05),
    "sharp_beta0.005": dict(beta=0.005),                     # the density is a near-step: compositing cancels
    "saturated_x3": dict(beta=0.05, boost=3.0),              # hidden SDF weights and latents x3: softplus saturates on both sides
    "scale_dist0.8": dict(beta=0.05, sd=0.8),                # both ends of the estimator's 1 +- size_range
    "scale_dist1.2": dict(beta=0.05, sd=1.2),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_training_render_float64_budget(golden, variant):
    """Training render B=4 x R=512 (131,072 points + 4,096 eikonal points, the G12 shape): outputs and every gradient tensor.

    Finding (class point_sum, K = 16): the gradients of the last SDF bias and of beta are sums of one term per sample point over all
    131,072 points.  The HIP reductions add fixed-order per-tile partials in fp32, torch adds in its blocked / vectorised order; both HIP
    arms sit at the same distance from float64 (g12: sdf.lin5.bias 3.5e-6 default, 2.8e-6 twins, 3.1e-7 fp32 oracle; sharp beta:
    density.beta 3.0e-5 / 5.0e-5 / 3.9e-6), so it is the summation order and not the split arithmetic.  These bars (<= 16 x the oracle's
    error, ~8e-5 of max) stay far inside the 2e-4 of test_gpu_parity_large.py.

    Limit: most other tensors are 1.0 +- 0.2 x the fp32 oracle in all three arms -- the error is dominated by the fp32 sample points
    and ray directions, which all three compute identically (render.hip reproduces torch's op order bit for bit), not by the MLP
    arithmetic.  A dropped third bf16 piece in the RGB reverse chain (2^-17 per weight) stays below that shared noise here; the kernel
    case test_rgb_composite_float64_budget, which starts from the same fp32 per-point inputs, catches it."""
    from oracle import reference_ops as R
    v = VARIANTS[variant]
    B, Rr = 4, 512
    opt, cfg = _opt(224, 224), R.Cfg(H=224, W=224)
    Ws, Wr = _g12_weights(golden)
    pose, intr, sd, zs, zr = _cameras(cfg, B, seed=7, sd=v.get("sd"))
    if v.get("boost"):
        Ws = {k: (t * v["boost"] if k in ("lin1.weight", "lin2.weight", "lin3.weight", "lin4.weight") else t) for k, t in Ws.items()}
        zs, zr = zs * v["boost"], zr * v["boost"]
    leaves = dict(pose=pose, intr=intr, scale_dist=sd, z_sdf=zs, z_rgb=zr)
    gen = torch.Generator().manual_seed(8)
    ray_idx = torch.stack([torch.randperm(224 * 224, generator=gen)[:Rr] for _ in range(B)])
    torch.manual_seed(1234)
    state = torch.get_rng_state()
    draws = R.draw_render_randoms(B * Rr, 64, True)
    cot = dict(rgb=torch.randn(B, Rr, 3, generator=gen), mask=torch.randn(B, Rr, 1, generator=gen),
               depth=torch.randn(B, Rr, 1, generator=gen), normal=torch.randn(B, Rr, 3, generator=gen),
               eik=torch.randn(2 * B * Rr, generator=gen))
    # normals only where the ray hits, as the loss uses them (one fp32 forward, no backward)
    hit = R.render(cfg, Ws, Wr, torch.tensor(v["beta"]), pose, intr, sd, zs, zr, ray_idx, True, *draws)["mask_hard"].detach()
    cot["normal"] = cot["normal"] * hit
    o32, g32 = _oracle_render(cfg, Ws, Wr, v["beta"], leaves, ray_idx, draws, cot, torch.float32)
    o64, g64 = _oracle_render(cfg, Ws, Wr, v["beta"], leaves, ray_idx, draws, cot, torch.float64)
    od, gd = _hip_render(opt, Ws, Wr, v["beta"], leaves, ray_idx, cot, state)
    with _twins():
        ot, gt = _hip_render(opt, Ws, Wr, v["beta"], leaves, ray_idx, cot, state)
    print("hit fraction %.2f" % float(o64["mask_hard"].mean()))
    _check("training render B=4 R=512 [%s]" % variant, _render_rows(o64, g64, o32, g32, od, gd, ot, gt), K_RENDER)


def test_eval_render_one_image_float64_budget(golden):
    """Evaluation render of one 48x48 image (147,456 points): rgb, mask, depth and the normals of rays that hit."""
    from oracle import reference_ops as R
    dev = torch.device("cuda:0")
    beta = 0.05
    opt, cfg = _opt(48, 48), R.Cfg(H=48, W=48)
    Ws, Wr = _g12_weights(golden)
    pose, intr, sd, zs, zr = _cameras(cfg, 1, seed=11)

    def hip():
        from shapeclipper_amd.model.implicit import RGBNetwork, SDFNetwork
        from shapeclipper_amd.model.renderer import Renderer
        sdf_net, rgb_net = SDFNetwork(opt), RGBNetwork(opt)
        sdf_net.load_state_dict(Ws)
        rgb_net.load_state_dict(Wr)
        r = Renderer(opt, sdf_net, rgb_net).to(dev)
        with torch.no_grad():
            r.density.beta.fill_(beta)
            o = r(opt, pose.to(dev), intr.to(dev), sd.to(dev), zs.to(dev), zr.to(dev), ray_idx=None, training=False)
        torch.cuda.synchronize()
        return dict(zip(("rgb", "mask", "mask_hard", "depth", "normal"), [x.cpu() for x in o[:5]]))
    od = hip()
    with _twins():
        ot = hip()
    ref = {}
    for dt in (torch.float32, torch.float64):
        _, eik_idx, _ = R.draw_render_randoms(48 * 48, 64, False)
        with R.default_dtype(dt), torch.no_grad():
            c = lambda t: t.to(dt)
            o = R.render(cfg, {k: c(v) for k, v in Ws.items()}, {k: c(v) for k, v in Wr.items()}, torch.tensor(beta), c(pose), c(intr),
                         c(sd), c(zs), c(zr), torch.arange(48 * 48).view(1, -1), False, None, eik_idx, None)
        ref[dt] = {k: o[k] for k in ("rgb", "mask", "mask_hard", "depth", "normal")}
    o64, o32 = ref[torch.float64], ref[torch.float32]
    hit = (o64["mask_hard"] > 0.5) & (o32["mask_hard"] > 0.5) & (od["mask_hard"] > 0.5) & (ot["mask_hard"] > 0.5)
    hit = hit & ((o64["mask"] - 0.5).abs() > 1e-3)
    rows = {}
    for k in ("rgb", "mask", "depth", "normal"):
        sel = (lambda x: x * hit) if k == "normal" else (lambda x: x)
        rows["out." + k] = ("out", _err(sel(od[k]), sel(o64[k])), _err(sel(ot[k]), sel(o64[k])), _err(sel(o32[k]), sel(o64[k])))
    print("hit fraction %.2f" % float(o64["mask_hard"].mean()))
    _check("evaluation render 48x48, one image", rows, K_RENDER)


# ---------------------------------------------------------------------------------------------------------------------------------
# kernel: the SDF backward (csrc/sdf_bwdw.hip, fused: n_per_image % 16 == 0), every weight, latent and point gradient
# ---------------------------------------------------------------------------------------------------------------------------------
K_SDF_BWD = dict(w_sdf=4.0, z=4.0, points=4.0)          # measured: <= 2.5 (w_sdf), 0.9 (z), 1.2 (points) x the fp32 oracle
# non-fused path (test_sdf_backward_nonfused_float64_budget) measured: <= 3.1 (w_sdf), 1.3 (z), 1.6 (points) x the fp32 oracle


def _sdf_bwd_oracle(cfg, W, z, pts, c, B, dt):
    """L = <sdf, c1> + <d sdf/dx, c2> + <feat, c3> through R.sdf_mlp with the latent attached, in dtype dt (double backward).  c2 / c3
    None: that term is absent (c2 None: no d sdf/dx at all, a single backward -- the value-only path of pretrain.py)."""
    from oracle import reference_ops as R
    with R.default_dtype(dt):
        Wl = {k: v.to(dt).clone().requires_grad_(True) for k, v in W.items()}
        zl, pl = z.to(dt).clone().requires_grad_(True), pts.to(dt).clone().requires_grad_(True)
        N = pts.shape[0] // B
        out = R.sdf_mlp(cfg, Wl, pl, zl.unsqueeze(1).repeat(1, N, 1).view(B * N, -1))
        sdf, feat = out[:, :1], out[:, 1:]
        L = (sdf[:, 0] * c[0].to(dt)).sum()
        if c[1] is not None:
            grad = torch.autograd.grad(sdf, pl, torch.ones_like(sdf), create_graph=True)[0]
            L = L + (grad * c[1].to(dt)).sum()
        if c[2] is not None:
            L = L + (feat * c[2].to(dt)).sum()
        gs = torch.autograd.grad(L, list(Wl.values()) + [zl, pl], allow_unused=True)
    return dict(zip(list(Wl) + ["z", "points"], [(x if x is not None else torch.zeros_like(v)).detach()
                                                   for x, v in zip(gs, list(Wl.values()) + [zl, pl])]))


def _sdf_bwd_hip(W, z, pts, c, N, symmetric=True, fused=True):
    """SdfFunction forward + backward; d sdf/dx is computed (and differentiated) only when c2 is given, the feature term only when
    c3 is given (otherwise g_feat is None in the backward)."""
    from shapeclipper_amd import packing
    from shapeclipper_amd.functional import SdfFunction
    dev = torch.device("cuda:0")
    Wd = {k: v.to(dev).requires_grad_(True) for k, v in W.items()}
    zd, pd = z.to(dev).requires_grad_(True), pts.to(dev).requires_grad_(True)
    pack, cb = packing.pack_sdf(Wd, zd)
    sdf, grad, feat = SdfFunction.apply(pd, pack, cb, N, symmetric, c[1] is not None, True, fused)
    L = (sdf * c[0].to(dev)).sum()
    if c[1] is not None:
        L = L + (grad * c[1].to(dev)).sum()
    if c[2] is not None:
        L = L + (packing.tbl_to_rows(feat, pts.shape[0]) * c[2].to(dev)).sum()
    gs = torch.autograd.grad(L, list(Wd.values()) + [zd, pd])
    torch.cuda.synchronize()
    return dict(zip(list(Wd) + ["z", "points"], [x.cpu() for x in gs]))


@pytest.mark.parametrize("B,N", [(1, 16), (3, 1040), (2, 40960)])      # one tile; tails and image boundaries; 2.5 persistent sweeps
def test_sdf_backward_fused_float64_budget(B, N):
    """sc_sdf_backward_fused (after the streamed / fp32 forward) against float64 double backward of R.sdf_mlp, same fp32 inputs.

    The fused backward has no fp32 twin: both HIP arms run the same kernel and differ only in the forward's parked activations, which
    test_sdf_forward_float64_budget holds to (a).  So only (b) applies here -- measured <= 1.4 x the fp32 oracle -- and (a) would compare
    two samples of the same rounding (at B=3 N=1040 lin3.weight: 1.6e-5 after the split forward, 8.1e-6 after the fp32 one, 1.5e-5 for
    the fp32 oracle)."""
    from oracle import reference_ops as R
    cfg = R.Cfg()
    g = torch.Generator().manual_seed(B * 7 + N)
    W = {k: v + 0.05 * torch.randn(v.shape, generator=g) for k, v in R.init_sdf_weights(cfg, 1).items()}
    z = torch.randn(B, 64, generator=g)
    pts = torch.rand(B * N, 3, generator=g) * 2 - 1
    c = (torch.randn(B * N, generator=g), torch.randn(B * N, 3, generator=g), torch.randn(B * N, 64, generator=g) * 0.1)
    r64, r32 = _sdf_bwd_oracle(cfg, W, z, pts, c, B, torch.float64), _sdf_bwd_oracle(cfg, W, z, pts, c, B, torch.float32)
    d = _sdf_bwd_hip(W, z, pts, c, N)
    with _twins():
        t = _sdf_bwd_hip(W, z, pts, c, N)
    rows = {k: ("w_sdf" if k.startswith("lin") else k, _err(d[k], r64[k]), _err(t[k], r64[k]), _err(r32[k], r64[k])) for k in r64}
    _check("SDF backward (fused) B=%d N=%d" % (B, N), rows, K_SDF_BWD, rule_a=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# the non-fused SDF backward: csrc/sdf_bwd.hip, 8 sc_wgrad launches, tbl_sum.  Production reaches it without any flag: pretrain.py
# (value only), the eikonal call of a training render when 2 R % 16 != 0, the per-point-latent SDFNetwork.forward (n_per_image = 1).
# ---------------------------------------------------------------------------------------------------------------------------------
NONFUSED = {
    "pretrain": (4, 10000, False),         # options/pix3d/config.yaml pre.sample_points; folded bias sums, fixed-order tbl_sum
    "fused_shape": (3, 1040, True),        # the inputs of test_sdf_backward_fused_float64_budget, fused=False; the fused arm beside it
    "ragged_eik": (3, 74, True),           # 2 R at R = 37: tiles straddle images, unfolded tbl_sum (atomics) for the latent biases
    "per_point_latent": (3000, 1, False),  # SDFNetwork.forward: one latent per point
}


@pytest.mark.parametrize("feat", [True, False])
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("case", list(NONFUSED))
def test_sdf_backward_nonfused_float64_budget(case, symmetric, feat):
    """sdf_bwd.hip + sc_wgrad + tbl_sum against float64 (double) backward of R.sdf_mlp, rule (b) with K_SDF_BWD.  Second arm: the
    fused backward on the same inputs where it applies (fused_shape), else the non-fused path after the fp32-MFMA forward.  feat=False
    leaves g_feat None: the W5 / B5 feature rows are the wrapper's zero fill."""
    from oracle import reference_ops as R
    B, N, with_grad = NONFUSED[case]
    cfg = R.Cfg(force_symmetry=symmetric)
    g = torch.Generator().manual_seed(B * 7 + N)
    W = {k: v + 0.05 * torch.randn(v.shape, generator=g) for k, v in R.init_sdf_weights(cfg, 1).items()}
    z = torch.randn(B, 64, generator=g)
    pts = torch.rand(B * N, 3, generator=g) * 2 - 1
    c = (torch.randn(B * N, generator=g), torch.randn(B * N, 3, generator=g), torch.randn(B * N, 64, generator=g) * 0.1)
    c = (c[0], c[1] if with_grad else None, c[2] if feat else None)
    r64, r32 = _sdf_bwd_oracle(cfg, W, z, pts, c, B, torch.float64), _sdf_bwd_oracle(cfg, W, z, pts, c, B, torch.float32)
    d = _sdf_bwd_hip(W, z, pts, c, N, symmetric, fused=False)
    if case == "fused_shape":
        second = "fused"
        t = _sdf_bwd_hip(W, z, pts, c, N, symmetric, fused=True)
    else:
        second = "non-fused after the fp32 forward"
        with _twins():
            t = _sdf_bwd_hip(W, z, pts, c, N, symmetric, fused=False)
    if not feat:
        assert float(d["lin5.weight"][1:].abs().max()) == 0.0 and float(d["lin5.bias"][1:].abs().max()) == 0.0
    rows = {k: ("w_sdf" if k.startswith("lin") else k, _err(d[k], r64[k]), _err(t[k], r64[k]), _err(r32[k], r64[k])) for k in r64}
    _check("SDF backward (non-fused) [%s] B=%d N=%d symmetric=%s feat=%s; columns: non-fused | %s | fp32 oracle"
           % (case, B, N, symmetric, feat, second), rows, K_SDF_BWD, rule_a=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# kernel: RGB network + compositing, forward and backward (split / fp32-stash forms) from the same fp32 per-point inputs
# ---------------------------------------------------------------------------------------------------------------------------------
# measured: <= 1.4 (out), 2.2 (w_rgb), 2.1 (latent) x the fp32 oracle; 3.9 (point): d L / d points runs through the derivative of the
# positional encoding, cos(2^k x) up to k = 5, which both HIP arms evaluate with the hardware sine / cosine and torch with libm.  With the
# third bf16 piece of the reverse chain dropped, the split arm's feature and point gradients are 14-53x its twin's: (a) fails.
K_RGB = dict(out=4.0, point=8.0, w_rgb=4.0, latent=4.0)


def _rgb_case(n_images, rpi, seed, S=64):
    """Per-point SDF results from the HIP forward (fp32), points off the rays: the compositing kernel only sees numbers.  S samples per ray."""
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
    ins = dict(points=pts, z_vals=z, depth_fac=dfac, sdf=sdf.cpu(), grad=grad.cpu(), feat=packing.tbl_to_rows(feat, n_rays * S).cpu(),
               beta=torch.tensor([0.1]))
    return cfg, ins, Wr, zr


def _rgb_oracle(cfg, ins, Wr, zr, rpi, cot, dt):
    """float64 / fp32 restatement of the compositing (R.rgb_mlp, R.laplace_density, R.volume_rendering, the sums of R.render)."""
    import torch.nn.functional as F
    from oracle import reference_ops as R
    S = ins["z_vals"].shape[1]
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


def _rgb_refs(n_images, rpi, S=64):
    """Inputs, the rays that hit, cotangents (normals only where a ray hits) and the float64 / fp32 oracle outputs and gradients."""
    cfg, ins, Wr, zr = _rgb_case(n_images, rpi, seed=n_images * 100 + rpi + (S - 64), S=S)
    n_rays = n_images * rpi
    o64, _ = _rgb_oracle(cfg, ins, Wr, zr, rpi, None, torch.float64)
    hit = (o64["mask"] - 0.5).abs() > 1e-3
    hit &= o64["mask"] > 0.5
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


@pytest.mark.parametrize("n_images,rpi", [(3, 40), (3, 37), (2, 512)])
def test_rgb_composite_float64_budget(n_images, rpi):
    """sc_rgb_composite_forward_split + backward_fused_split (default) / forward_stash + the fp32 fused backward (twins) against a float64
    restatement that starts from the same fp32 points, z_vals, depth factors, sdf, d sdf/dx, features and weights."""
    (ins, Wr, zr, hit, cot), ref = _rgb_refs(n_images, rpi)
    od, gd = _rgb_hip(ins, Wr, zr, rpi, cot)
    with _twins():
        ot, gt = _rgb_hip(ins, Wr, zr, rpi, cot)
    assert torch.equal(od["mask_hard"], ot["mask_hard"])
    print("hit fraction %.2f" % float(hit.float().mean()))
    _check("RGB composite n_images=%d rays/image=%d" % (n_images, rpi), _rgb_rows(ref, hit, od, gd, ot, gt), K_RGB)


@contextmanager
def _switches(**kw):
    """ops module switches set for the block and restored however it exits."""
    from shapeclipper_amd import ops
    saved = {k: getattr(ops, k) for k in kw}
    try:
        for k, v in kw.items():
            setattr(ops, k, v)
        yield
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)


@contextmanager
def _count_wgrad():
    """Counts the sc_wgrad launches of ops (the RGB backward without in-kernel weight gradients makes three)."""
    from shapeclipper_amd import ops
    calls, real = [], ops._wgrad

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)
    ops._wgrad = spy
    try:
        yield calls
    finally:
        ops._wgrad = real


# --hip.fused_rgb_wgrad!: sc_rgb_composite_backward_v3 + 3 sc_wgrad launches; --hip.rgb_stash!: the fused backward recomputes the forward.
# measured at (3, 40), (3, 37) and (2, 512): <= 1.4 (out), 3.4 (point), 2.1 (w_rgb), 2.1 (latent) x the fp32 oracle -- the default path's factors.
# 257 images (test_rgb_composite_257_images_float64_budget) measured: <= 1.4 (out), 4.3 (point), 3.7 (w_rgb), 1.4 (latent).
RGB_ALTS = {"fused_rgb_wgrad_off": (dict(FUSED_RGB_WGRAD=False), 3), "rgb_stash_off": (dict(RGB_STASH=False), 0)}


# Finding (fixed): both alternates recompute the RGB forward chain inside the backward (rgb_composite_bwd_kernel without STASH).  The
# recomputation evaluated the positional encoding with the hardware sine / cosine, the forward with the accurate sincosf; the ~1e-6 difference
# moved pre-activations near zero across the ReLU kink, so the backward's masks were not the forward's.  At 2 images x 512 rays that put
# points 3.5e-4, feat 4.3e-4, lin0 / lin1 weights and biases 2.7e-5 .. 6.6e-5 and z_rgb 2.2e-5 of max off float64 (points 1300x, feat 1270x,
# lin1.bias 550x, z_rgb 115x the fp32 oracle) while lin2, lin3, the outputs and the compositing gradients matched.  The recomputation now
# uses the accurate sincosf: test_rgb_backward_recomputes_the_forward_activations_bit_for_bit.
@pytest.mark.parametrize("alt", list(RGB_ALTS))
@pytest.mark.parametrize("n_images,rpi", [(3, 40), (3, 37), (2, 512)])
def test_rgb_composite_alternate_backward_float64_budget(n_images, rpi, alt):
    """The RGB backward's alternate paths on the inputs of test_rgb_composite_float64_budget, rule (b) with K_RGB; columns: default |
    alternate | fp32 oracle."""
    kw, n_wgrad = RGB_ALTS[alt]
    (ins, Wr, zr, hit, cot), ref = _rgb_refs(n_images, rpi)
    od, gd = _rgb_hip(ins, Wr, zr, rpi, cot)
    with _switches(**kw), _count_wgrad() as calls:
        ot, gt = _rgb_hip(ins, Wr, zr, rpi, cot)
    assert len(calls) == n_wgrad
    assert torch.equal(od["mask_hard"], ot["mask_hard"])
    _check("RGB composite n_images=%d rays/image=%d; columns: default | %s | fp32 oracle" % (n_images, rpi, alt),
           _rgb_rows(ref, hit, od, gd, ot, gt), K_RGB, rule_a=False)


@pytest.mark.parametrize("n_images,rpi", [(3, 37), (2, 512)])
def test_rgb_backward_recomputes_the_forward_activations_bit_for_bit(n_images, rpi):
    """sc_rgb_composite_backward_v3 recomputes the RGB chain and hands r0, r1 to sc_wgrad: they must be bit-equal to what the fp32 forward
    (sc_rgb_composite_forward_stash, the same rgb_chain) parks, so that the backward's ReLU masks are the forward's."""
    import ctypes
    from shapeclipper_amd import _lib, ops, packing
    dev = torch.device("cuda:0")
    cfg, ins, Wr, zr = _rgb_case(n_images, rpi, seed=n_images * 100 + rpi)
    x = {k: (packing.rows_to_tbl(v) if k == "feat" else v).to(dev).contiguous() for k, v in ins.items()}
    v_pack, dbias = packing.pack_rgb({k: v.to(dev) for k, v in Wr.items()}, zr.to(dev))
    args = (x["points"], x["z_vals"], x["depth_fac"], x["sdf"], x["grad"], x["feat"], v_pack, dbias, x["beta"])
    with _switches(RGB_FWD_SPLIT=False):
        o = ops.rgb_composite_forward(*args, rpi, True, 1e-4, 1.0, 1.0, keep_rgb_flat=True, keep_rr=True)
    n_rays = n_images * rpi
    P, T = n_rays * 64, n_rays * 4 * 1024
    g = torch.Generator().manual_seed(rpi)
    G = [torch.randn(n_rays, 3, generator=g), torch.randn(n_rays, generator=g), torch.randn(n_rays, generator=g),
         torch.randn(n_rays, 3, generator=g)]
    G = [t.to(dev) for t in G]
    e = lambda *shape: torch.empty(*shape, device=dev)
    outs = [e(P), e(P, 3), e(T), e(P, 3), e(n_rays, 64), e(n_rays), e(ops.RGB_BWD_BETA_PARTS)]
    gy, rr = e(3 * T), torch.full((2 * T,), float("nan"), device=dev)
    v3_part = e(ops.RGB_BWD_BETA_PARTS * 196)
    lib = _lib.load()
    code = lib.sc_rgb_composite_backward_v3(*[_lib.ptr(t) for t in args + (o["rgb_flat"],)], ctypes.c_int(n_rays), ctypes.c_int(rpi),
                                            ctypes.c_int(n_images), ctypes.c_int(1), ctypes.c_float(1e-4), ctypes.c_float(1.0),
                                            ctypes.c_float(1.0), *[_lib.ptr(t) for t in G], *[_lib.ptr(t) for t in outs], _lib.ptr(gy),
                                            _lib.ptr(rr), None, _lib.ptr(v3_part), _lib.stream())
    assert code == 0
    torch.cuda.synchronize()
    fwd = o["rr"][:2 * T]
    n_diff = int((rr.view(torch.int32) != fwd.view(torch.int32)).sum())
    print("recomputed r0, r1 differing from the forward's: %d of %d" % (n_diff, 2 * T))
    assert n_diff == 0


def test_rgb_composite_257_images_float64_budget():
    """257 images (4 rays each): past the 256-image limit of the fused backward, so the default switches take
    sc_rgb_composite_backward_v3 + 3 sc_wgrad launches (ops.rgb_composite_backward) and the forward parks no activations.  Columns:
    default | twins | fp32 oracle."""
    n_images, rpi = 257, 4
    (ins, Wr, zr, hit, cot), ref = _rgb_refs(n_images, rpi)
    with _count_wgrad() as calls:
        od, gd = _rgb_hip(ins, Wr, zr, rpi, cot)
    assert len(calls) == 3
    with _twins():
        ot, gt = _rgb_hip(ins, Wr, zr, rpi, cot)
    _check("RGB composite n_images=257 rays/image=4", _rgb_rows(ref, hit, od, gd, ot, gt), K_RGB, rule_a=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# kernel: ray sampling (csrc/render.hip ray_sample_kernel / ray_sample_bwd_kernel), plain and with the eikonal points
# ---------------------------------------------------------------------------------------------------------------------------------
K_RAY = dict(leaf=4.0)          # measured: <= 2.2 x fp32 torch autograd (larger ratios only below the 2^-22 floor)


def _ray_restated(o, d, sd, u, eik_idx, R, dist):
    """UniformSampler.get_z_vals + the sample points + the near-surface eikonal points, as torch ops in the inputs' dtype."""
    n = d.shape[0]
    c = (dist * sd).repeat_interleave(R).view(n, 1)
    near, far = c - 0.7, c + 0.7
    t = torch.linspace(0.0, 1.0, steps=64).to(d.device, d.dtype)
    z = near * (1.0 - t) + far * t
    if u is not None:
        mids = 0.5 * (z[..., 1:] + z[..., :-1])
        upper = torch.cat([mids, z[..., -1:]], -1)
        lower = torch.cat([z[..., :1], mids], -1)
        z = lower + (upper - lower) * u.to(d.dtype)
    pts = (o.unsqueeze(1) + z.unsqueeze(2) * d.unsqueeze(1)).reshape(-1, 3)
    near_pts = pts.view(n, 64, 3)[torch.arange(n, device=d.device), eik_idx]
    return z, pts, near_pts


def _ray_case(B, R, training, seed):
    g = torch.Generator().manual_seed(seed)
    n = B * R
    o = torch.randn(n, 3, generator=g)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    sd = 0.8 + 0.4 * torch.rand(B, generator=g)
    u = torch.rand(n, 64, generator=g) if training else None
    eik_idx = torch.randint(64, (n,), generator=g)
    eik_idx[0], eik_idx[-1] = (63, 0) if n > 1 else ((63,) * 2 if training else (0,) * 2)
    eik_u = torch.rand(n, 3, generator=g) * 2 - 1
    cot = dict(z=torch.randn(n, 64, generator=g), pts=torch.randn(n * 64, 3, generator=g), eik=torch.randn(B, 2 * R, 3, generator=g))
    return o, d, sd, u, eik_idx, eik_u, cot


@pytest.mark.parametrize("eik", [True, False])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B,R", [(1, 1), (3, 37), (2, 1000), (32, 512)])
def test_ray_sample_float64_budget(B, R, training, eik):
    """RaySampleEikFunction / RaySampleFunction.  Forward: z and the points bit-equal to the fp32 torch restatement, the eikonal points
    bit-equal to [eik_uniform | points[ray, eik_idx]] per image.  Backward: g_cam_loc, g_ray_dirs and the per-image g_scale_dist (a sum
    of R x 64 terms) against float64 autograd of the restatement, rule (b) against fp32 torch autograd."""
    from shapeclipper_amd.functional import RaySampleEikFunction, RaySampleFunction
    dev = torch.device("cuda:0")
    dist = 5.0
    o, d, sd, u, eik_idx, eik_u, cot = _ray_case(B, R, training, seed=B * 1000 + R + training)
    n = B * R
    leaf = lambda t, dt=torch.float32, dv=dev: t.to(dv, dt).clone().requires_grad_(True)
    od, dd, sdd = leaf(o), leaf(d), leaf(sd)
    ud = u.to(dev) if u is not None else None
    cz, cp, ce = cot["z"].to(dev), cot["pts"].to(dev), cot["eik"].to(dev)
    if eik:
        z, p, e = RaySampleEikFunction.apply(od, dd, sdd, ud, eik_idx.to(dev), eik_u.to(dev), R, dist)
        L = (z * cz).sum() + (p * cp).sum() + (e * ce).sum()
    else:
        z, p = RaySampleFunction.apply(od, dd, sdd, ud, R, dist)
        L = (z * cz).sum() + (p * cp).sum()
    gh = [x.cpu() for x in torch.autograd.grad(L, [od, dd, sdd])]
    # fp32 torch restatement on the device: the forward bit for bit, and the fp32 autograd arm
    o32, d32, sd32 = leaf(o), leaf(d), leaf(sd)
    zr, pr, nr = _ray_restated(o32, d32, sd32, ud, eik_idx.to(dev), R, dist)
    assert torch.equal(z, zr) and torch.equal(p, pr)
    L32 = (zr * cz).sum() + (pr * cp).sum()
    if eik:
        assert torch.equal(e, torch.cat([eik_u.to(dev).view(B, R, 3), nr.view(B, R, 3)], 1))
        L32 = L32 + (nr.view(B, R, 3) * ce[:, R:]).sum()
    g32 = [x.cpu() for x in torch.autograd.grad(L32, [o32, d32, sd32])]
    torch.cuda.synchronize()
    # float64 autograd from the same fp32 inputs
    cpu = torch.device("cpu")
    o64, d64, sd64 = leaf(o, torch.float64, cpu), leaf(d, torch.float64, cpu), leaf(sd, torch.float64, cpu)
    z64, p64, n64 = _ray_restated(o64, d64, sd64, u.double() if u is not None else None, eik_idx, R, dist)
    L64 = (z64 * cot["z"].double()).sum() + (p64 * cot["pts"].double()).sum()
    if eik:
        L64 = L64 + (n64.view(B, R, 3) * cot["eik"][:, R:].double()).sum()
    g64 = torch.autograd.grad(L64, [o64, d64, sd64])
    rows = {k: ("leaf", _err(a, r), _err(a, r), _err(b, r)) for k, a, b, r in zip(("g_cam_loc", "g_ray_dirs", "g_scale_dist"), gh, g32, g64)}
    _check("ray sampling B=%d R=%d training=%s eik=%s; columns: HIP | HIP | fp32 torch" % (B, R, training, eik), rows, K_RAY, rule_a=False)
