"""The surface render: csrc/surface_hit.hip (ops.ray_first_crossing, ops.ray_bracket_step), Renderer.render_surface / render_views(surface=True)
and `--hip.surface_render`.

The rule for the two kernels: every output is bit-identical to the numpy restatement of the header's text (tests/surface_hit_ref.py).
render_surface is compared, bit for bit as well, with its own chain spelled out here from the existing ops and those restatements.
Shapes: 130 rays (two full groups of 64 and a remainder; 33 workgroups of 4 waves) at every chunk count S / 64 the kernels walk, 16 x 16
images of a geometric-init sphere of radius 0.5 (about half of the rays hit it).  The one figure that is measured, not derived -- the
median |sdf| at the surface point with and without refinement -- is printed and only its ordering is asserted."""
import ctypes
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import surface_hit_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEV = torch.device("cuda:0")
N_RAYS = 130
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
host = lambda t: t.detach().cpu().numpy()


def _same(got, want, what):
    got = host(got) if isinstance(got, torch.Tensor) else got
    bad = int((np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)).sum()) if got.shape == want.shape else -1
    print("%s: %d of %d elements differ" % (what, bad, want.size))
    assert got.dtype == want.dtype and bad == 0, what


def _same_bracket(got, want, what):
    for name, g, w in zip(ref.Bracket._fields, got, want):
        _same(g, w, "%s %s" % (what, name))


# ---- the crossing kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [32, 64, 96, 128, 256])
def test_first_crossing_matches_the_restatement_bit_for_bit(S):
    from shapeclipper_amd import ops
    for iso in (0.0, 0.5):
        z, sdf, want_rows = ref.crossing_case(S, N_RAYS, iso=iso)
        want = ref.first_crossing(z, sdf, iso)
        zd, sd = dev(z), dev(sdf)
        keep = (zd.clone(), sd.clone())
        got = ops.ray_first_crossing(zd, sd, iso)
        assert isinstance(got, ops.RayBracket) and got.hit.dtype == torch.int32 and all(t.shape == (N_RAYS,) for t in got)
        _same_bracket(got, want, "S=%d iso=%g" % (S, iso))
        assert torch.equal(zd, keep[0]) and torch.equal(sd.view(torch.int32), keep[1].view(torch.int32))     # the inputs are not written
        hit = host(got.hit)
        for k, (h, i) in enumerate(want_rows):                      # the crafted rows give what their names say, on the device too
            name = ref.crafted_rows(S)[k][0]
            assert hit[k] == h, (S, iso, name)
            if i is not None:
                assert host(got.t_lo)[k] == z[k, i] and host(got.t_hi)[k] == z[k, i + 1], (S, iso, name)
        print("S=%d iso=%g: hit codes 0/1/2 = %s" % (S, iso, np.bincount(hit, minlength=3).tolist()))
        assert {0, 1, 2} <= set(hit.tolist())


def test_first_crossing_one_ray_and_an_empty_batch():
    from shapeclipper_amd import ops
    z, sdf, _ = ref.crossing_case(64, N_RAYS)
    for n in (1, 3, 4, 5):
        _same_bracket(ops.ray_first_crossing(dev(z[:n]), dev(sdf[:n * 64])), ref.first_crossing(z[:n], sdf[:n * 64]), "n_rays=%d" % n)
    got = ops.ray_first_crossing(torch.empty(0, 64, device=DEV), torch.empty(0, device=DEV))
    assert all(t.shape == (0,) for t in got)


# ---- the step kernel ----------------------------------------------------------------------------------------------------------------------
def _dev_bracket(br):
    from shapeclipper_amd import ops
    return ops.RayBracket(*(dev(a) for a in br))


def test_bracket_step_matches_the_restatement_and_keeps_its_invariants():
    from shapeclipper_amd import ops
    br, cam, d = ref.step_case(N_RAYS)
    camd, dd = dev(cam), dev(d)
    got = _dev_bracket(br)
    one = br.hit == 1
    # f_new NULL: the first query, the bracket untouched
    t, p = ops.ray_bracket_step(got, camd, dd)
    want_br, want_t, want_p = ref.bracket_step(br, cam, d)
    _same(t, want_t, "step 0 t"); _same(p, want_p, "step 0 points"); _same_bracket(got, br, "step 0 bracket (untouched)")
    assert host(t)[0] == br.t_lo[0] + np.float32(0.5) * (br.t_hi[0] - br.t_lo[0])          # the overflowing difference bisects
    assert host(t)[1] == br.t_lo[1] + np.float32(0.5) * (br.t_hi[1] - br.t_lo[1])          # f_lo = +Inf too
    assert np.isfinite(host(p)).all()
    for k in range(6):                                              # f_new positive, negative, zero, NaN, +-Inf, huge: step_values
        f = ref.step_values(want_t, k)
        prev = want_br
        want_br, want_t2, want_p = ref.bracket_step(want_br, cam, d, f, want_t)
        t2, p = ops.ray_bracket_step(got, camd, dd, dev(f), t)
        _same(t2, want_t2, "step %d t" % (k + 1)); _same(p, want_p, "step %d points" % (k + 1)); _same_bracket(got, want_br, "step %d bracket" % (k + 1))
        g = [host(a) for a in got]
        assert (g[0][one] <= host(t2)[one]).all() and (host(t2)[one] <= g[1][one]).all()                  # t_lo <= t <= t_hi
        assert (g[2][one] > 0).all() and (g[3][one] <= 0).all()                                          # f_lo > 0 >= f_hi
        assert (g[0][one] >= prev.t_lo[one]).all() and (g[1][one] <= prev.t_hi[one]).all()               # the bracket never widens
        for a, b in zip(g[:4], br[:4]):                                                                  # hit != 1 rays never move
            assert np.array_equal(a[~one].view(np.uint32), b[~one].view(np.uint32))
        assert np.array_equal(host(t2)[~one], br.t_lo[~one])
        moved = int(((g[0] != prev.t_lo) | (g[1] != prev.t_hi)).sum())
        print("step %d: %d of %d hit == 1 brackets moved, widest now %g" % (k + 1, moved, int(one.sum()), float((g[1] - g[0])[one].max())))
        t, want_t = t2, want_t2
    # t_prev may be the tensor that receives t; iso shifts f_new
    br2, t0 = _dev_bracket(br), dev(ref.bracket_step(br, cam, d)[1])
    f = ref.step_values(host(t0), 0) + np.float32(0.25)
    w_br, w_t, w_p = ref.bracket_step(br, cam, d, f, host(t0), iso=0.25)
    t2, p = ops.ray_bracket_step(br2, camd, dd, dev(f), t0, iso=0.25)
    _same(t2, w_t, "iso t"); _same(p, w_p, "iso points"); _same_bracket(br2, w_br, "iso bracket")


# ---- render_surface -----------------------------------------------------------------------------------------------------------------------
B, H, W = 3, 16, 16


@functools.lru_cache(maxsize=None)
def _scene():
    """(opt, renderer, pose [B,3,4], intr [B,3,3], scale_dist [B], latent_sdf, latent_rgb): the geometric-init SDF network (a sphere of
    radius 0.5), a random RGB network, three cameras around it.  Built once and left unchanged."""
    from oracle import reference_ops as R
    from shapeclipper_amd.model.implicit import RGBNetwork, SDFNetwork
    from shapeclipper_amd.model.renderer import Renderer
    from shapeclipper_amd.utils import options
    opt = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_surface_gpu",
                                               "--output_root=/tmp/sc_pytest"]), verbose=False)
    opt.H, opt.W = H, W
    assert opt.arch.impl_sdf.geometric_init and opt.arch.impl_sdf.init_sphere_radius == 0.5 and opt.render.n_samples_uniform == 64
    torch.manual_seed(0)
    sdf_net, rgb_net = SDFNetwork(opt), RGBNetwork(opt)
    r = Renderer(opt, sdf_net, rgb_net).to(DEV).eval()
    cfg = R.Cfg(H=H, W=W)
    trig = lambda t: torch.stack([torch.cos(t), torch.sin(t)], 1)
    sd = torch.tensor([0.9, 1.0, 1.1])
    pose = R.pose_from_trig(cfg, trig(torch.tensor([0.3, -1.1, 2.0])), trig(torch.tensor([0.2, -0.1, 0.4])), trig(torch.zeros(B)), sd)
    intr = R.get_intr(cfg, torch.tensor([1.0, 1.1, 0.95]))
    zs, zr = torch.randn(B, 64) * 0.3, torch.randn(B, 64)
    return opt, r, pose.to(DEV).contiguous(), intr.to(DEV).contiguous(), sd.to(DEV), zs.to(DEV), zr.to(DEV)


def _chain(n_refine, k=1, images=slice(None), kernels=False):
    """render_surface's chain spelled out: the existing ops and, for the two new kernels, their numpy restatements (kernels=True: the
    kernels themselves, for the residual measurement) -> dict of numpy outputs, the surface points and z_vals."""
    from shapeclipper_amd import ops
    opt, r, pose, intr, sd, zs, zr = _scene()
    pose, intr, sd, zs, zr = pose[images], intr[images], sd[images], zs[images], zr[images]
    n, S, R = pose.shape[0], r.N_samples, k * k * H * W
    sym = bool(r.sdf_network.force_symmetry)
    with torch.no_grad():
        w_pack, cbias = r.sdf_network.packed(zs)
        v_pack, dbias = r.rgb_network.packed(zr)
        intr_k = (intr * torch.tensor([k, k, 1.0], device=DEV).view(1, 3, 1)).contiguous()
        cam, dirs, dfac = ops.camera_rays_forward(pose.contiguous(), intr_k, None, R, k * W)
        z, pts = ops.ray_sample_forward(cam, dirs, sd.contiguous(), None, R, float(opt.camera.dist), S)
        value = lambda p, per: ops.sdf_forward(p, w_pack, cbias, per, symmetric=sym, want_grad=False, want_feat=False)[0]
        sdf = value(pts, R * S)
        if kernels:
            br = ops.ray_first_crossing(z, sdf)
            t, p = ops.ray_bracket_step(br, cam, dirs)
            for _ in range(n_refine):
                t, p = ops.ray_bracket_step(br, cam, dirs, value(p, R), t)
            hit, t = host(br.hit), host(t)
        else:
            camn, dirn = host(cam), host(dirs)
            br, t, p = ref.bracket_step(ref.first_crossing(host(z), host(sdf)), camn, dirn)
            for _ in range(n_refine):
                br, t, p = ref.bracket_step(br, camn, dirn, host(value(dev(p), R)), t)
            hit, p = br.hit, dev(p)
        _, grad, feat = ops.sdf_forward(p, w_pack, cbias, R, symmetric=sym, want_grad=True, want_feat=True)
        rgb, normal = ops.rgb_points_forward(p, grad, feat, v_pack, dbias, R, sym)
        residual = host(value(p, R))
    m = (hit != 0)[:, None]
    f32 = np.float32
    return dict(rgb=np.where(m, host(rgb), f32(opt.data.bgcolor)).astype(f32).reshape(n, R, 3), mask=m.astype(f32).reshape(n, R, 1),
                depth=np.where(m, (t * host(dfac))[:, None], f32(0)).astype(f32).reshape(n, R, 1),
                normal=np.where(m, host(normal), f32(0)).astype(f32).reshape(n, R, 3), hit=hit.reshape(n, R).astype(np.int32),
                residual=residual.reshape(n, R), z=host(z).reshape(n, R, S), dfac=host(dfac).reshape(n, R, 1))


def _render(n_refine=3, k=1, images=slice(None)):
    opt, r, pose, intr, sd, zs, zr = _scene()
    return r.render_surface(opt, pose[images], intr[images], sd[images], zs[images], zr[images], n_refine=n_refine, scale=k)


def _same_render(got, want, what):
    for name in ("rgb", "mask", "depth", "normal", "hit"):
        _same(getattr(got, name), want[name] if isinstance(want, dict) else host(getattr(want, name)), "%s %s" % (what, name))


@pytest.mark.parametrize("n_refine", [0, 3])
def test_render_surface_equals_its_chain_spelled_out(n_refine):
    from shapeclipper_amd.model.renderer import SurfaceRender
    opt = _scene()[0]
    rng = torch.get_rng_state()
    got = _render(n_refine)
    assert torch.equal(torch.get_rng_state(), rng)                                  # draws nothing
    assert isinstance(got, SurfaceRender) and got._fields == ("rgb", "mask", "depth", "normal", "hit")
    assert got.rgb.shape == (B, H * W, 3) and got.mask.shape == (B, H * W, 1) and got.depth.shape == (B, H * W, 1)
    assert got.normal.shape == (B, H * W, 3) and got.hit.shape == (B, H * W) and got.hit.dtype == torch.int32
    want = _chain(n_refine)
    _same_render(got, want, "n_refine=%d" % n_refine)
    hit, rgb, mask, depth, normal = (host(getattr(got, k)) for k in ("hit", "rgb", "mask", "depth", "normal"))
    miss = hit == 0
    assert miss.any() and (hit == 1).any()
    assert (rgb[miss] == np.float32(opt.data.bgcolor)).all() and (mask[miss] == 0).all() and (depth[miss] == 0).all() and (normal[miss] == 0).all()
    assert np.array_equal(mask[..., 0] != 0, hit != 0) and set(np.unique(mask).tolist()) <= {0.0, 1.0}
    lo, hi = want["z"][..., :1] * want["dfac"], want["z"][..., -1:] * want["dfac"]
    assert ((depth >= lo) & (depth <= hi))[~miss].all()
    n = np.linalg.norm(normal[~miss], axis=-1)
    print("n_refine=%d: hit codes %s, |normal| on hits in [%.7f, %.7f]" % (n_refine, np.bincount(hit.ravel(), minlength=3).tolist(), n.min(), n.max()))
    assert np.abs(n - 1).max() < 1e-5 and np.isfinite(rgb).all()


def test_refinement_does_not_raise_the_residual():
    """The median |sdf| at the surface point over the hit == 1 rays, with three refinement rounds against none.  Only the ordering is asserted:
    nobody has derived a bound for the residual.  Both medians are printed (run with -s)."""
    med = {}
    for n_refine in (0, 3):
        c = _chain(n_refine, kernels=True)
        one = c["hit"] == 1
        assert one.sum() * 4 >= one.size, (int(one.sum()), one.size)                # at least a quarter of the rays bracket a crossing
        med[n_refine] = float(np.median(np.abs(c["residual"][one])))
        print("n_refine=%d: %d of %d rays hit == 1, median |sdf(p)| = %.4g, max %.4g" % (n_refine, int(one.sum()), one.size, med[n_refine],
                                                                                       float(np.abs(c["residual"][one]).max())))
    assert med[3] <= med[0], med


def test_an_image_does_not_depend_on_its_batch_or_the_stream():
    full = _render(3)
    for b in range(B):
        one = _render(3, images=slice(b, b + 1))
        for name in full._fields:
            assert torch.equal(getattr(one, name)[0], getattr(full, name)[b]), (b, name)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _render(3)
    again = _render(3)
    torch.cuda.synchronize()
    for o in (other, again):
        for name in full._fields:
            assert torch.equal(getattr(o, name), getattr(full, name)), name


def test_scale_one_shoots_the_evaluation_rays_and_scale_two_four_times_as_many(monkeypatch):
    from shapeclipper_amd import ops
    from shapeclipper_amd.functional import CameraRaysFunction
    opt, r, pose, intr, sd, zs, zr = _scene()
    seen = []
    step = ops.ray_bracket_step
    monkeypatch.setattr(ops, "ray_bracket_step", lambda br, cam, dirs, *a, **k: seen.append((cam, dirs)) or step(br, cam, dirs, *a, **k))
    _render(0, k=1)
    cam, dirs, _ = CameraRaysFunction.apply(pose, intr, None, H * W, W)
    assert len(seen) == 1 and torch.equal(seen[0][0], cam) and torch.equal(seen[0][1], dirs)
    monkeypatch.undo()
    got = _render(3, k=2)
    R = 4 * H * W
    assert got.rgb.shape == (B, R, 3) and got.mask.shape == (B, R, 1) and got.depth.shape == (B, R, 1) and got.normal.shape == (B, R, 3)
    assert got.hit.shape == (B, R)
    _same_render(got, _chain(3, k=2), "scale=2")
    # the same view: the mask at twice the resolution, pooled 2 x 2, agrees with the scale-1 mask away from the silhouette
    m1 = _render(3).mask.view(B, H, W)
    m2 = got.mask.view(B, H, 2, W, 2).mean(dim=(2, 4))
    agree = float(((m2 > 0.5) == (m1 > 0.5)).float().mean())
    print("scale 2 pooled against scale 1: %.3f of the pixels agree" % agree)
    assert agree > 0.9


def test_surface_turntable_equals_the_view_by_view_loop():
    from oracle import reference_ops as R
    opt, r, pose, intr, sd, zs, zr = _scene()
    V = 5
    trig = lambda t: torch.stack([torch.cos(t), torch.sin(t)], 1)
    az = torch.linspace(0, 2 * np.pi, V + 1)[:V]
    poses = R.pose_from_trig(R.Cfg(H=H, W=W), trig(az), trig(torch.full((V,), 0.3)), trig(torch.zeros(V)), torch.ones(V)).to(DEV).contiguous()
    ones = torch.ones(B, device=DEV)
    loop = [r.render_surface(opt, poses[v:v + 1].expand(B, 3, 4).contiguous(), intr, ones, zs, zr, n_refine=3, scale=1) for v in range(V)]
    for chunk in (None, 1, 2, V):
        got = r.render_views(opt, poses, intr, zs, zr, chunk_views=chunk, surface=True, n_refine=3, scale=1)
        assert got.rgb.shape == (V, B, H * W, 3) and got.hit.shape == (V, B, H * W)
        for v in range(V):
            for name in got._fields:
                assert torch.equal(getattr(got, name)[v], getattr(loop[v], name)), (chunk, v, name)
    small = r.render_views(opt, poses, intr, zs, zr, max_rays=H * W, surface=True)            # one image per pass inside the chain
    assert all(torch.equal(a, b) for a, b in zip(small, got))
    assert not torch.equal(got.rgb[0], got.rgb[2])                                            # the views differ (colours: the solid is a near-sphere)
    rgb, mask, normal = r.render_views(opt, poses, intr, zs, zr)                              # the volume turn-table keeps its call and result
    assert rgb.shape == (V, B, H * W, 3) and mask.shape == (V, B, H * W, 1) and normal.shape == (V, B, H * W, 3)


# ---- the raw C ABI ------------------------------------------------------------------------------------------------------------------------
def test_raw_c_abi_writes_n_rays_elements_and_nothing_else():
    from shapeclipper_amd import _lib
    lib = _lib.load()
    S, n, G = 96, 37, 64                                             # guard: G elements on either side of every output
    z, sdf, _ = ref.crossing_case(S, n)
    want = ref.first_crossing(z, sdf)
    zd, sd = dev(z), dev(sdf)

    def guarded(count, dtype=torch.float32):
        t = torch.full((count + 2 * G,), 0x5a5a5a5a, device=DEV, dtype=torch.int32)
        return t, t[G:G + count].view(dtype)

    def intact(t, count):
        return bool((t[:G] == 0x5a5a5a5a).all()) and bool((t[G + count:] == 0x5a5a5a5a).all())

    p, ci, cf = _lib.ptr, ctypes.c_int, ctypes.c_float
    bufs = [guarded(n) for _ in range(4)] + [guarded(n, torch.int32)]
    rc = lib.sc_ray_first_crossing(p(zd), p(sd), ci(n), ci(S), cf(0.0), *(p(v) for _, v in bufs), _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0
    for (whole, view), w, name in zip(bufs, want, ref.Bracket._fields):
        _same(view, w, "C ABI crossing %s" % name)
        assert intact(whole, n), name
    br, cam, d = ref.step_case(n)
    camd, dd = dev(cam), dev(d)
    bb = [guarded(n) for _ in range(4)] + [guarded(n, torch.int32)]
    for (_, view), a in zip(bb, br):
        view.copy_(dev(a))
    tw, tv = guarded(n)
    pw, pv = guarded(3 * n)
    rc = lib.sc_ray_bracket_step(p(camd), p(dd), None, None, ci(n), cf(0.0), *(p(v) for _, v in bb), p(tv), p(pv), _lib.stream())
    assert rc == 0
    w_br, w_t, w_p = ref.bracket_step(br, cam, d)
    _same(tv, w_t, "C ABI step t"); _same(pv.view(n, 3), w_p, "C ABI step points")
    f = ref.step_values(w_t, 1)
    rc = lib.sc_ray_bracket_step(p(camd), p(dd), p(dev(f)), p(tv), ci(n), cf(0.0), *(p(v) for _, v in bb), p(tv), p(pv), _lib.stream())   # t_prev == t
    torch.cuda.synchronize()
    assert rc == 0
    w_br, w_t, w_p = ref.bracket_step(w_br, cam, d, f, w_t)
    _same(tv, w_t, "C ABI step 2 t"); _same(pv.view(n, 3), w_p, "C ABI step 2 points")
    for (whole, view), w, name in zip(bb, w_br, ref.Bracket._fields):
        _same(view, w, "C ABI step 2 %s" % name)
        assert intact(whole, n), name
    assert intact(tw, n) and intact(pw, 3 * n)
    # refused calls launch nothing
    assert lib.sc_ray_first_crossing(p(zd), p(sd), ci(n), ci(48), cf(0.0), *(p(v) for _, v in bufs), _lib.stream()) == 1
    assert lib.sc_ray_first_crossing(p(zd), p(sd), ci(n), ci(S), cf(0.0), None, *(p(v) for _, v in bufs[1:]), _lib.stream()) == 1
    assert lib.sc_ray_bracket_step(p(camd), p(dd), p(dev(f)), None, ci(n), cf(0.0), *(p(v) for _, v in bb), p(tv), p(pv), _lib.stream()) == 1
    assert lib.sc_ray_first_crossing(p(zd), p(sd), ci(0), ci(S), cf(0.0), *(p(v) for _, v in bufs), _lib.stream()) == 0
    torch.cuda.synchronize()


# ---- end to end: the Runner's dumps --------------------------------------------------------------------------------------------------------
def _opt(extra, output_root):
    from shapeclipper_amd.utils import options
    return options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_surface_render", "--output_root=%s" % output_root,
                                                "--arch.enc_pretrained!", "--data.dataset=synthetic", "--eval.num_points=5000", "--tb!", *extra]),
                       verbose=False)


def _runner(o):
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    from shapeclipper_amd.model.runner import Runner
    o.device, o.world_size, o.port = 0, 1, 0
    torch.manual_seed(0)
    r = Runner(o)
    r.load_dataset(o, eval_split="test")
    r.build_networks(o)
    r.graph.eval()
    return r


def _tree(path):
    out = {}
    for base, _, files in os.walk(path):
        for f in files:
            out[os.path.relpath(os.path.join(base, f), path)] = open(os.path.join(base, f), "rb").read()
    return out


SURFACE_FILES = ("image_surface.png", "mask_surface.png", "normal_surface.png", "depth_surface.png", "depth_surface.npy")


def test_evaluation_writes_the_five_files_and_changes_nothing_else(tmp_path, monkeypatch):
    from PIL import Image
    from shapeclipper_amd.model.renderer import Renderer
    k = 2
    o = _opt(["--hip.surface_render", "--hip.surface_scale=%d" % k], str(tmp_path))
    r = _runner(o)
    n = len(r.test_data)
    Hk, Wk = k * o.eval.image_size[0], k * o.eval.image_size[1]
    depths = []
    render = Renderer.render_surface
    monkeypatch.setattr(Renderer, "render_surface", lambda self, *a, **kw: depths.append(render(self, *a, **kw)) or depths[-1])
    trees = {}
    for mode in ("evaluate", "evaluate_sharded"):
        del depths[:]
        o.hip.surface_render = True
        getattr(r, mode)(o, ep=0)
        on = _tree(o.output_path)
        assert len(depths) == n
        depth = torch.cat([d.depth for d in depths]).view(n, Hk, Wk).cpu().numpy()
        hit = torch.cat([d.hit for d in depths]).view(n, Hk, Wk).cpu().numpy()
        for i in range(n):
            for f in SURFACE_FILES:
                assert "dump/%d_%s" % (i, f) in on, (mode, i, f)
            for f in SURFACE_FILES[:4]:
                im = Image.open(os.path.join(o.output_path, "dump", "%d_%s" % (i, f)))
                assert im.size == (Wk, Hk), (mode, f, im.size)
            saved = np.load(os.path.join(o.output_path, "dump", "%d_depth_surface.npy" % i))
            assert saved.dtype == np.float32 and saved.shape == (Hk, Wk) and np.array_equal(saved.view(np.uint32), depth[i].view(np.uint32)), (mode, i)
            grey = np.asarray(Image.open(os.path.join(o.output_path, "dump", "%d_depth_surface.png" % i)))
            assert grey.shape == (Hk, Wk) and (grey[hit[i] == 0] == 255).all()                           # misses are white
            mask = np.asarray(Image.open(os.path.join(o.output_path, "dump", "%d_mask_surface.png" % i)))
            assert np.array_equal(mask == 255, hit[i] != 0) and np.array_equal(mask == 0, hit[i] == 0)
        # the switch off: nothing is rendered, the surface files are gone, everything else keeps its bytes
        for f in on:
            if f.startswith("dump/"):
                os.remove(os.path.join(o.output_path, f))
        del depths[:]
        o.hip.surface_render = False
        getattr(r, mode)(o, ep=0)
        off = _tree(o.output_path)
        assert depths == []
        extra = sorted(set(on) - set(off))
        assert extra == sorted("dump/%d_%s" % (i, f) for i in range(n) for f in SURFACE_FILES), (mode, extra)
        assert set(off) <= set(on)
        for f in ("chamfer.txt", "f_score.txt"):
            assert f in off
        for f, data in off.items():
            assert on[f] == data, (mode, f)
        for f in off:
            if f.startswith("dump/"):
                os.remove(os.path.join(o.output_path, f))
        trees[mode] = on
    for i in range(n):                                                                                    # sharded or not: the same pictures
        for f in SURFACE_FILES:
            name = "dump/%d_%s" % (i, f)
            assert trees["evaluate"][name] == trees["evaluate_sharded"][name], name


def test_train_vis_dump_gets_the_five_files_and_two_turntable_gifs(tmp_path):
    from PIL import Image
    from shapeclipper_amd.model.graph import Graph
    from shapeclipper_amd.model.runner import Runner
    from shapeclipper_amd.utils.util import EasyDict as edict
    opt, r, pose, intr, sd, zs, zr = _scene()
    o = edict(opt)
    o.hip = edict(opt.hip)
    o.hip.surface_render, o.hip.surface_scale, o.hip.surface_refine = True, 2, 2
    o.output_path = str(tmp_path)
    V = 5
    var = edict(idx=torch.tensor([4, 9, 11], device=DEV), pose=pose, intr=intr, scale_dist=sd, proj_latent_sdf=zs, proj_latent_rgb=zr,
                rgb_input_map=torch.zeros(B, 3, 2, 2, device=DEV))
    Graph.get_rotate_pose(None, o, var, n_views=V)
    runner = types.SimpleNamespace(graph=types.SimpleNamespace(module=types.SimpleNamespace(renderer=r)))
    os.makedirs(os.path.join(o.output_path, "vis_3"))
    Runner.dump_surface(runner, o, var, "vis_3", rotate=True)
    files = sorted(os.listdir(os.path.join(o.output_path, "vis_3")))
    want = sorted("%d_%s" % (i, f) for i in (4, 9, 11) for f in SURFACE_FILES + ("image_surface_rotate.gif", "normal_surface_rotate.gif"))
    assert files == want
    for i in (4, 9, 11):
        for g in ("image_surface_rotate", "normal_surface_rotate"):
            gif = Image.open(os.path.join(o.output_path, "vis_3", "%d_%s.gif" % (i, g)))
            assert gif.size == (2 * W, 2 * H) and 1 < gif.n_frames <= V, (i, g)
        assert np.load(os.path.join(o.output_path, "vis_3", "%d_depth_surface.npy" % i)).shape == (2 * H, 2 * W)
        assert Image.open(os.path.join(o.output_path, "vis_3", "%d_normal_surface.png" % i)).size == (2 * W, 2 * H)
