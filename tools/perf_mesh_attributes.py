"""Coloured mesh dump cost: eval_3D.mesh_attributes (marching cubes + SDF gradient/feature + RGB chain at the vertices) against
ops.isosurface_mesh alone, and ops.rgb_points_forward alone at the same vertices, timed with device events after warm-up, alternating,
in one process.  A geometric-init SDF network (a sphere of radius 0.5, zero latent) and an RGB network with random weights; vox_res 100
and 256, B = 1 and 8 level grids.
python tools/perf_mesh_attributes.py [--iters N]"""
import argparse, json, os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch


def _time(f, iters):
    ms = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); f(); e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return sorted(ms)[len(ms) // 2], min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    from shapeclipper_amd import ops
    from shapeclipper_amd.model.implicit import RGBNetwork, SDFNetwork
    from shapeclipper_amd.utils import eval_3D, options
    from shapeclipper_amd.utils.util import EasyDict as edict
    dev = torch.device("cuda:0")
    opt = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=perf_mesh_attributes",
                                               "--output_root=/tmp/sc_perf"]), verbose=False)
    torch.manual_seed(0)
    sdf_net, rgb_net = SDFNetwork(opt).to(dev), RGBNetwork(opt).to(dev)
    with torch.no_grad():
        for p in rgb_net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    lo, hi = opt.eval.range
    for vox in (100, 256):
        opt.eval.vox_res = vox
        for B in (1, 8):
            with torch.no_grad():
                zs = torch.zeros(B, opt.arch.impl_sdf.proj_latent_dim, device=dev)
                zr = torch.randn(B, opt.arch.impl_rgb.proj_latent_dim, device=dev)
                var = edict(idx=torch.arange(B, device=dev))
                level = eval_3D.compute_level_grid(opt, sdf_net, zs, eval_3D.get_dense_3D_grid(opt, var))
                S = level.shape[1]
                verts, _, vc, _ = ops.isosurface_mesh(level)
                q = (lo + verts * ((hi - lo) / (S - 1))).contiguous()
                P = 16 * ((int(vc.max()) + 15) // 16)
                # the kernel alone: one image's worth of rows per image, as mesh_attributes lays them out (no padding needed to time it)
                n = q.shape[0]
                w_pack, cbias = sdf_net.packed(zs[:1])
                _, grad, feat = ops.sdf_forward(q, w_pack, cbias, 16 * ((n + 15) // 16), symmetric=True)
                v_pack, dbias = rgb_net.packed(zr[:1])
                runs = {"isosurface_mesh": lambda: ops.isosurface_mesh(level),
                        "mesh_attributes": lambda: eval_3D.mesh_attributes(opt, sdf_net, rgb_net, zs, zr, level),
                        "rgb_points_forward": lambda: ops.rgb_points_forward(q, grad, feat, v_pack, dbias, 16 * ((n + 15) // 16), True)}
                for f in runs.values():                                    # warm-up: code objects, allocator
                    f(); f()
                torch.cuda.synchronize()
                res = {k: _time(f, a.iters) for k, f in runs.items()}
            print(json.dumps(dict(vox_res=vox, images=B, vertices=int(vc.sum()), rows=B * P,
                                  **{k + "_ms": round(v[0], 4) for k, v in res.items()},
                                  **{k + "_ms_best": round(v[1], 4) for k, v in res.items()},
                                  attributes_over_mesh_ms=round(res["mesh_attributes"][0] - res["isosurface_mesh"][0], 4),
                                  iters=a.iters)), flush=True)
            del level, verts, q, grad, feat
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
