"""Renderer.render_surface timed with device events beside the volume evaluation render (Renderer.forward(training=False)) of the same
networks, cameras and H x W, in one process on one device.

Configurations: B = 1 and B = 32 images of --size x --size pixels (default 128, the evaluation render of tools/workloads.py), surface
render at scale k = 1, 2 with n_refine = 0, 3.  The networks are the geometric-init sphere (radius 0.5) with a small perturbation, seen
from cameras around it: about half of the rays hit.  Every figure is the median of --iters event-timed calls after two warm-up calls of
that configuration (code objects, allocator); the volume render is timed before and after the surface configurations of a batch size.
One JSON line per configuration, then the per-launch split of the surface render at k = 1, n_refine = 3 (each stage of the chain timed
on its own with events, the others still enqueued around it).  Per-kernel times: run this tool under `rocprofv3 --kernel-trace --stats`
(the two new kernels are ray_first_crossing_kernel and ray_bracket_step_kernel).
python tools/perf_surface_render.py [--iters N] [--size 128]"""
import argparse, json, os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch


def timed(fn, iters):
    fn(); fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    ms.sort()
    return round(ms[len(ms) // 2], 4), round(ms[0], 4)


def cameras(opt, B, dev):
    from shapeclipper_amd.model.graph import rotation_from_trig
    from shapeclipper_amd.utils import camera
    trig = lambda t: torch.stack([torch.cos(t), torch.sin(t)], 1)
    az, el = torch.linspace(0, 5.5, B), torch.linspace(-0.3, 0.5, B)
    R = rotation_from_trig(trig(az), trig(el), trig(torch.zeros(B)))
    sd = torch.linspace(0.9, 1.1, B)
    pose_R = camera.pose(R=R)
    pose_T = camera.pose(t=torch.stack([torch.zeros(B), torch.zeros(B), sd * opt.camera.dist], -1))
    pose = camera.pose.compose([pose_R, pose_T])
    return pose.to(dev).contiguous(), camera.get_intr(opt, torch.ones(B)).to(dev).contiguous(), sd.to(dev)


def split(r, opt, pose, intr, sd, zs, zr, n_refine, iters):
    """Median event time of every stage of the k = 1 chain, in the order render_surface enqueues them."""
    from shapeclipper_amd import ops
    from shapeclipper_amd.functional import CameraRaysFunction, RaySampleFunction
    R, S, sym = opt.H * opt.W, r.N_samples, bool(r.sdf_network.force_symmetry)
    w_pack, cbias = r.sdf_network.packed(zs)
    v_pack, dbias = r.rgb_network.packed(zr)
    value = lambda p, per: ops.sdf_forward(p, w_pack, cbias, per, symmetric=sym, want_grad=False, want_feat=False)[0]
    cam, dirs, dfac = CameraRaysFunction.apply(pose, intr, None, R, int(opt.W))
    z, pts = RaySampleFunction.apply(cam, dirs, sd, None, R, float(opt.camera.dist), S)
    sdf = value(pts, R * S)
    br = ops.ray_first_crossing(z, sdf)
    t, p = ops.ray_bracket_step(br, cam, dirs)
    f = value(p, R)
    _, grad, feat = ops.sdf_forward(p, w_pack, cbias, R, symmetric=sym)
    rgb, normal = ops.rgb_points_forward(p, grad, feat, v_pack, dbias, R, sym)
    hit = (br.hit != 0).unsqueeze(-1)

    def compose():
        torch.where(hit, rgb, torch.full_like(rgb, 1.0)); hit.float(); torch.where(hit, (t * dfac).unsqueeze(-1), torch.zeros_like(hit, dtype=torch.float32))
        torch.where(hit, normal, torch.zeros_like(normal))
    stages = [("camera rays", 1, lambda: CameraRaysFunction.apply(pose, intr, None, R, int(opt.W))),
              ("ray samples (R S points)", 1, lambda: RaySampleFunction.apply(cam, dirs, sd, None, R, float(opt.camera.dist), S)),
              ("SDF value at R S points", 1, lambda: value(pts, R * S)),
              ("ray_first_crossing", 1, lambda: ops.ray_first_crossing(z, sdf)),
              ("ray_bracket_step", n_refine + 1, lambda: ops.ray_bracket_step(br, cam, dirs, f, t)),
              ("SDF value at R points", n_refine, lambda: value(p, R)),
              ("SDF value + gradient + feature at R points", 1, lambda: ops.sdf_forward(p, w_pack, cbias, R, symmetric=sym)),
              ("rgb_points_forward", 1, lambda: ops.rgb_points_forward(p, grad, feat, v_pack, dbias, R, sym)),
              ("compose outputs (torch.where x 3, cast, multiply)", 1, compose)]
    return [dict(stage=name, calls=n, ms_each=timed(fn, iters)[0]) for name, n, fn in stages]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--size", type=int, default=128)
    a = ap.parse_args()
    from shapeclipper_amd.model.implicit import RGBNetwork, SDFNetwork
    from shapeclipper_amd.model.renderer import Renderer
    from shapeclipper_amd.utils import options
    dev = torch.device("cuda:0")
    opt = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=perf_surface_render",
                                               "--output_root=/tmp/sc_perf"]), verbose=False)
    opt.H = opt.W = a.size
    torch.manual_seed(0)
    sdf_net, rgb_net = SDFNetwork(opt), RGBNetwork(opt)
    with torch.no_grad():
        for net, scale in ((sdf_net, 0.003), (rgb_net, 0.03)):
            for p in net.parameters():
                p.add_(scale * torch.randn_like(p))
    r = Renderer(opt, sdf_net, rgb_net).to(dev).eval()
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), H=opt.H, W=opt.W, S=r.N_samples, iters=a.iters,
                          note="medians (and best) of device-event times in ms, two warm-up calls per configuration, one process")), flush=True)
    with torch.no_grad():
        for B in (1, 32):
            pose, intr, sd = cameras(opt, B, dev)
            zs, zr = torch.randn(B, 64, device=dev) * 0.3, torch.randn(B, 64, device=dev)
            volume = lambda: r(opt, pose, intr, sd, zs, zr, training=False)
            vol_before = timed(volume, a.iters)
            rows = []
            for k in (1, 2):
                for n_refine in (0, 3):
                    out = r.render_surface(opt, pose, intr, sd, zs, zr, n_refine=n_refine, scale=k)
                    ms = timed(lambda: r.render_surface(opt, pose, intr, sd, zs, zr, n_refine=n_refine, scale=k), a.iters)
                    rows.append(dict(B=B, scale=k, n_refine=n_refine, pixels="%dx%d" % (k * opt.H, k * opt.W), surface_ms=ms[0], surface_ms_best=ms[1],
                                     hit_fraction=round(float((out.hit != 0).float().mean()), 4)))
                    del out
            vol_after = timed(volume, a.iters)
            for row in rows:
                row.update(volume_ms_same_HxW=vol_before[0], volume_ms_same_HxW_after=vol_after[0],
                           volume_over_surface=round(vol_before[0] / row["surface_ms"], 2))
                print(json.dumps(row), flush=True)
            print(json.dumps(dict(B=B, scale=1, n_refine=3, split=split(r, opt, pose, intr, sd, zs, zr, 3, a.iters))), flush=True)


if __name__ == "__main__":
    main()
