"""Textured mesh bake cost: eval_3D.mesh_texture (marching cubes + texel queries + SDF gradient/feature + RGB chain at every texel of the
atlas rows that hold a face + pack + the centroid self-check) against eval_3D.mesh_attributes (the same chain at the vertices only) on
the same level grid, at eval.texture_texels T = 4, 8, 16; and the three kernels of csrc/texture_bake.hip alone.  Timed with device
events after warm-up, alternating, in one process.  A geometric-init SDF network (a sphere of radius 0.5, zero latent) and an RGB
network with random weights; vox_res 64 (the shipped setting) and 100, B = 1 level grid.  Prints the self-check of every bake as well.
python tools/perf_texture.py [--iters N] [--vox 64 100]"""
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
    ap.add_argument("--vox", type=int, nargs="+", default=[64, 100])
    a = ap.parse_args()
    from shapeclipper_amd import ops
    from shapeclipper_amd.model.implicit import RGBNetwork, SDFNetwork
    from shapeclipper_amd.utils import eval_3D, options
    from shapeclipper_amd.utils.util import EasyDict as edict
    dev = torch.device("cuda:0")
    opt = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=perf_texture",
                                               "--output_root=/tmp/sc_perf"]), verbose=False)
    torch.manual_seed(0)
    sdf_net, rgb_net = SDFNetwork(opt).to(dev), RGBNetwork(opt).to(dev)
    with torch.no_grad():
        for p in rgb_net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    lo, hi = opt.eval.range
    B = 1
    for vox in a.vox:
        opt.eval.vox_res = vox
        with torch.no_grad():
            zs = torch.zeros(B, opt.arch.impl_sdf.proj_latent_dim, device=dev)
            zr = torch.randn(B, opt.arch.impl_rgb.proj_latent_dim, device=dev)
            level = eval_3D.compute_level_grid(opt, sdf_net, zs, eval_3D.get_dense_3D_grid(opt, edict(idx=torch.arange(B, device=dev))))
            S = level.shape[1]
            verts, faces, vc, fc = ops.isosurface_mesh(level)
            F = fc.tolist()
            for T in (4, 8, 16):
                opt.eval.texture_texels = T
                A, n, rows = ops.texture_layout(max(F), T)
                q, fot = ops.texture_queries(verts, faces, [0], [0], F, A, T, lo, hi, S, rows)
                rgb, nrm = torch.rand_like(q), torch.nn.functional.normalize(torch.randn_like(q), dim=1)
                atlas, _ = ops.texture_pack(rgb, nrm, fot, A, rows)
                uv = eval_3D.texture_face_uv(F[0], A, T, dev).mean(dim=1).contiguous()
                image = torch.zeros(F[0], dtype=torch.int32, device=dev)
                runs = {"mesh_attributes": lambda: eval_3D.mesh_attributes(opt, sdf_net, rgb_net, zs, zr, level),
                        "mesh_texture": lambda: eval_3D.mesh_texture(opt, sdf_net, rgb_net, zs, zr, level),
                        "texture_queries": lambda: ops.texture_queries(verts, faces, [0], [0], F, A, T, lo, hi, S, rows),
                        "texture_pack": lambda: ops.texture_pack(rgb, nrm, fot, A, rows),
                        "texture_sample": lambda: ops.texture_sample(atlas, uv, image)}
                for f in runs.values():                                    # warm-up: code objects, allocator
                    f(); f()
                torch.cuda.synchronize()
                res = {k: _time(f, a.iters) for k, f in runs.items()}
                stats = eval_3D.mesh_texture(opt, sdf_net, rgb_net, zs, zr, level)[0].stats
                print(json.dumps(dict(vox_res=vox, texels=T, faces=F[0], vertices=int(vc.sum()), atlas=A, rows=rows, queried_texels=rows * A,
                                      used_texels=int((fot >= 0).sum()),
                                      **{k + "_ms": round(v[0], 4) for k, v in res.items()},
                                      **{k + "_ms_best": round(v[1], 4) for k, v in res.items()},
                                      texture_over_attributes=round(res["mesh_texture"][0] / res["mesh_attributes"][0], 2),
                                      err_mean=round(stats["err_mean"], 4), err_max=round(stats["err_max"], 4), iters=a.iters)), flush=True)
                del q, fot, rgb, nrm, atlas
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
