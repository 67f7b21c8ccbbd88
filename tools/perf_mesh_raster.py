"""Rasteriser cost: ops.mesh_raster and eval_3D.mesh_render (raster + the two atlas look-ups) of the vox_res 64 marching-cubes mesh of a
geometric-init SDF network (a sphere of radius 0.5, slightly perturbed), B = 1: one 224 x 224 view and the 50-view turn-table, at
large_pixels = the default (64), 2^40 (every face by its own thread: the wave kernel finds empty lists) and 0 (every face by a wave),
and the share of the default's time that the wave path accounts for, (default - threads only) / default.  Beside them, on the same
device in the same run and at the same pixel count: Renderer.render_surface (one view) and Renderer.render_views(surface=True) (the
turn-table), the renders that look at the same SDF without a mesh.  Timed with device events after warm-up, medians.
python tools/perf_mesh_raster.py [--iters N] [--size 224] [--views 50]"""
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
    return round(ms[len(ms) // 2], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--views", type=int, default=50)
    a = ap.parse_args()
    from shapeclipper_amd import ops
    from shapeclipper_amd.model.graph import Graph
    from shapeclipper_amd.model.implicit import RGBNetwork, SDFNetwork
    from shapeclipper_amd.model.renderer import Renderer
    from shapeclipper_amd.utils import camera, eval_3D, options
    from shapeclipper_amd.utils.util import EasyDict as edict
    dev = torch.device("cuda:0")
    opt = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=perf_mesh_raster",
                                               "--output_root=/tmp/sc_perf", "--eval.vox_res=64"]), verbose=False)
    opt.H = opt.W = a.size
    torch.manual_seed(0)
    sdf_net, rgb_net = SDFNetwork(opt), RGBNetwork(opt)
    with torch.no_grad():
        for net, scale in ((sdf_net, 0.003), (rgb_net, 0.03)):
            for p in net.parameters():
                p.add_(scale * torch.randn_like(p))
    r = Renderer(opt, sdf_net, rgb_net).to(dev).eval()
    B, H, W = 1, a.size, a.size
    with torch.no_grad():
        zs, zr = torch.zeros(B, 64, device=dev), torch.randn(B, 64, device=dev)
        var = edict(idx=torch.arange(B, device=dev), intr=camera.get_intr(opt, torch.ones(B)).to(dev), scale_dist=torch.ones(B, device=dev),
                    rgb_input_map=torch.zeros(B, 3, 2, 2, device=dev))
        Graph.get_rotate_pose(None, opt, var, n_views=a.views)
        turn = var.vis_pose.contiguous()                                    # [V,3,4]
        one = turn[:1].contiguous()                                         # [B,3,4]
        level = eval_3D.compute_level_grid(opt, sdf_net, zs, eval_3D.get_dense_3D_grid(opt, var))
        textured = eval_3D.mesh_texture(opt, sdf_net, rgb_net, zs, zr, level)
        lo, hi = opt.eval.range
        S = level.shape[1]
        verts, faces, vc, fc = ops.isosurface_mesh(level)
        world = (lo + verts * ((hi - lo) / (S - 1))).contiguous()
        F = fc.tolist()
        row = dict(device=torch.cuda.get_device_name(0), vox_res=S, faces=F[0], vertices=int(vc.sum()), H=H, W=W, views=a.views, iters=a.iters)
        for name, pose in (("one_view", one[:, None].contiguous()), ("turntable", turn[None].contiguous())):
            raster = lambda lp: ops.mesh_raster(world, faces, [0], [0], F, pose, var.intr, H, W, eval_3D.MESH_RENDER_NEAR, large_pixels=lp)
            out = raster(ops.RASTER_LARGE_PIXELS)
            t = {k: timed(lambda: raster(lp), a.iters) for k, lp in (("default", ops.RASTER_LARGE_PIXELS), ("threads_only", 1 << 40), ("waves_only", 0))}
            row.update({"%s_raster_ms_%s" % (name, k): v for k, v in t.items()})
            row["%s_wave_path_share" % name] = round((t["default"] - t["threads_only"]) / t["default"], 4)
            row["%s_covered_fraction" % name] = round(float((out.face >= 0).float().mean()), 4)
            row["%s_mesh_render_ms" % name] = timed(lambda: eval_3D.mesh_render(opt, level, textured, pose, var.intr, H, W), a.iters)
        row["one_view_render_surface_ms"] = timed(lambda: r.render_surface(opt, one, var.intr, var.scale_dist, zs, zr), a.iters)
        row["turntable_render_views_surface_ms"] = timed(lambda: r.render_views(opt, turn, var.intr, zs, zr, surface=True), max(3, a.iters // 3))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
