"""The oracle as a float64 restatement (oracle/reference_ops.py follows torch's default dtype): under
``R.default_dtype(torch.float64)`` the training render computes in float64 throughout, agrees with the fp32 render to fp32
rounding, and the default dtype is restored however the block exits.  The float64 run is the yardstick of
tests/test_gpu_float64_budget.py and tests/test_gpu_non_finite.py."""
import pytest
import torch


def test_default_dtype_is_restored_after_an_exception():
    from oracle import reference_ops as R
    before = torch.get_default_dtype()
    with pytest.raises(RuntimeError):
        with R.default_dtype(torch.float64):
            assert torch.get_default_dtype() == torch.float64 and torch.zeros(1).dtype == torch.float64
            raise RuntimeError("inside")
    assert torch.get_default_dtype() == before == torch.float32


def _render(R, dt, seed=0, B=2, Rr=24):
    cfg = R.Cfg(H=32, W=32)
    g = torch.Generator().manual_seed(seed)
    Ws = R.init_sdf_weights(cfg, 1)
    Wr = R.init_rgb_weights(cfg, 2)
    Ws = {k: v + 0.01 * torch.randn(v.shape, generator=g) for k, v in Ws.items()}
    trig = lambda t: torch.stack([torch.cos(t), torch.sin(t)], 1)
    az, el, sd = torch.rand(B, generator=g) * 6 - 3, torch.rand(B, generator=g) - 0.5, 0.9 + 0.2 * torch.rand(B, generator=g)
    zs, zr = torch.randn(B, 64, generator=g) * 0.3, torch.randn(B, 64, generator=g) * 0.3
    centre = torch.tensor([y * 32 + x for y in range(8, 24) for x in range(8, 24)])      # the init sphere covers the centre of the frame
    ray_idx = torch.stack([centre[torch.randperm(256, generator=g)[:Rr]] for _ in range(B)])
    torch.manual_seed(seed)
    t_rand, eik_idx, eik_pts = R.draw_render_randoms(B * Rr, 64, True)          # fp32 draws in both runs
    with R.default_dtype(dt):
        c = lambda t: t.to(dt).clone().requires_grad_(True)
        Ws, Wr = {k: c(v) for k, v in Ws.items()}, {k: c(v) for k, v in Wr.items()}
        beta = c(torch.tensor(0.1))
        lv = dict(trig_azim=c(trig(az)), trig_elev=c(trig(el)), scale_dist=c(sd), z_sdf=c(zs), z_rgb=c(zr))
        pose = R.pose_from_trig(cfg, lv["trig_azim"], lv["trig_elev"], trig(torch.zeros(B)).to(dt), lv["scale_dist"])
        intr = R.get_intr(cfg, torch.ones(B))
        o = R.render(cfg, Ws, Wr, beta, pose, intr, lv["scale_dist"], lv["z_sdf"], lv["z_rgb"], ray_idx, True,
                     t_rand.to(dt), eik_idx, eik_pts.to(dt))
        L = o["rgb"].sum() + o["mask"].sum() + o["depth"].sum() + o["normal"].sum() + o["grad_eikonal"].sum()
        leaves = dict([("sdf." + k, v) for k, v in Ws.items()] + [("rgb." + k, v) for k, v in Wr.items()] + [("beta", beta)] + list(lv.items()))
        grads = torch.autograd.grad(L, list(leaves.values()))
    outs = {k: o[k].detach() for k in ("rgb", "mask", "depth", "normal", "grad_eikonal", "mask_hard")}
    return outs, dict(zip(leaves, grads))


def test_float64_render_agrees_with_fp32_render_to_fp32_rounding():
    from oracle import reference_ops as R
    o32, g32 = _render(R, torch.float32)
    o64, g64 = _render(R, torch.float64)
    assert torch.get_default_dtype() == torch.float32
    assert all(v.dtype == torch.float64 for v in o64.values()) and all(v.dtype == torch.float64 for v in g64.values())
    assert all(v.dtype == torch.float32 for v in o32.values())
    rel = lambda a, b: float((a.double() - b).abs().max() / max(float(b.abs().max()), 1e-30))
    hit = (o64.pop("mask_hard") > 0.5) & (o32.pop("mask_hard") > 0.5)
    assert hit.any()
    # the normal of a ray that misses is the normalised sum of weights ~1e-6: rounding noise in either precision
    o32["normal"], o64["normal"] = o32["normal"] * hit, o64["normal"] * hit
    eo = {k: rel(o32[k], o64[k]) for k in o64}
    eg = {k: rel(g32[k], g64[k]) for k in g64}
    print("fp32 vs float64 oracle, outputs:", {k: "%.1e" % v for k, v in eo.items()})
    print("fp32 vs float64 oracle, gradients:", {k: "%.1e" % v for k, v in eg.items()})
    # fp32 rounding (2^-24 = 6e-8 per operation) accumulated over a 64-sample composite / a few thousand-term weight sums
    assert max(eo.values()) < 1e-4, eo       # measured: <= 1.2e-5 (normal)
    assert max(eg.values()) < 2e-4, eg       # measured: <= 4.4e-5 (trig_elev)
    # ... and really a different computation: the float64 run is not the fp32 one widened
    assert max(eo.values()) > 0.0 and max(eg.values()) > 0.0
