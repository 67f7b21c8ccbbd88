"""Cost of the ambient occlusion of `--mesh.ao`: ops.level_ambient_occlusion (csrc/level_ao.hip: the bit volume of the occupied cells, then
one wave per point and one lane per direction marching the level grid) at vox_res 64 and 128, B = 1, at the default reach
(mesh.ao_radius 0.125 of the grid, samples half a pitch apart) -- on the vertices of the marching-cubes mesh and on the texels of a
T = 8 atlas, with cell_skip on and off -- beside ops.isosurface_mesh and eval_3D.mesh_attributes on the same level grid: a sphere (the
geometric-init SDF network: convex, every ray runs its whole length) and a torus (analytic: the hole occludes).  Normals are the grid's
central differences at the nearest grid point.  Device events around windows of `reps` calls (reps sized so that a window is at least
--window-ms long), after warm-up, the runs alternating, in one process; medians and bests per call (each call of the op ends with the
host read of its flag, so the figure is the op as the evaluation pays for it).  One JSON line per case.
python tools/perf_ao.py [--iters N] [--window-ms T] [--res 64,128] [--radius 0.125]"""
import argparse, json, os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch

from perf_mesh_stats import _time, level_grid


def grid_normals(level, points):
    """Central differences of level [S,S,S] at the grid point nearest to each of points [N,3] (grid-index units): [N,3] fp32."""
    S = level.shape[0]
    g = torch.stack(torch.gradient(level), dim=-1)
    i = points.round().long().clamp(0, S - 1)
    return g[i[:, 0], i[:, 1], i[:, 2]].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--res", default="64,128")
    ap.add_argument("--radius", type=float, default=0.125)
    ap.add_argument("--texels", type=int, default=8)
    a = ap.parse_args()
    from shapeclipper_amd import ops
    from shapeclipper_amd.model.implicit import RGBNetwork, SDFNetwork
    from shapeclipper_amd.utils import eval_3D, options
    from shapeclipper_amd.utils.util import EasyDict as edict
    dev = torch.device("cuda:0")
    opt = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=perf_ao", "--output_root=/tmp/sc_perf",
                                               "--mesh.ao", "--mesh.ao_radius=%r" % a.radius]), verbose=False)
    torch.manual_seed(0)
    sdf_net, rgb_net = SDFNetwork(opt).to(dev), RGBNetwork(opt).to(dev)
    lo, hi = opt.eval.range
    T = a.texels
    for S in (int(v) for v in a.res.split(",")):
        opt.eval.vox_res = S
        with torch.no_grad():
            zs = torch.zeros(1, opt.arch.impl_sdf.proj_latent_dim, device=dev)
            zr = torch.randn(1, opt.arch.impl_rgb.proj_latent_dim, device=dev)
            net = eval_3D.compute_level_grid(opt, sdf_net, zs, eval_3D.get_dense_3D_grid(opt, edict(idx=torch.arange(1, device=dev))))
        for kind, level in (("sphere", net.float().contiguous()), ("torus", level_grid("torus", 1, S, lo, hi, dev))):
            radius = options.ao_settings(opt, S)
            M = ops.ao_step_count(radius, eval_3D.AO_STEP)
            mesh = ops.isosurface_mesh(level)
            v_start, f_start, F = mesh.starts()
            A, _, rows = ops.texture_layout(max(F), T)
            query, fot = ops.texture_queries(mesh.verts, mesh.faces, v_start, f_start, F, A, T, lo, hi, S, rows)
            texels = ((query[fot.reshape(-1) >= 0] - lo) * ((S - 1) / (hi - lo))).contiguous()
            sets = {"vertices": mesh.verts.contiguous(), "atlas": texels}
            normals = {k: grid_normals(level[0], p) for k, p in sets.items()}
            image = {k: torch.zeros(len(p), dtype=torch.int32, device=dev) for k, p in sets.items()}
            ao = lambda k, skip: ops.level_ambient_occlusion(level, sets[k], normals[k], image[k], radius, step=eval_3D.AO_STEP,
                                                             bias=eval_3D.AO_BIAS, cell_skip=skip)
            runs = {"ao_vertices_skip": lambda: ao("vertices", True), "ao_vertices_noskip": lambda: ao("vertices", False),
                    "ao_atlas_skip": lambda: ao("atlas", True), "ao_atlas_noskip": lambda: ao("atlas", False),
                    "isosurface_mesh": lambda: ops.isosurface_mesh(level),
                    "mesh_attributes": lambda: eval_3D.mesh_attributes(opt, sdf_net, rgb_net, zs, zr, level)}
            same = all(torch.equal(x, y) for k in sets for x, y in zip(ao(k, True), ao(k, False)))
            reps = {}
            for name, f in runs.items():                                        # warm-up, then the size of a window
                f(); f()
                torch.cuda.synchronize()
                reps[name] = max(1, min(1000, int(a.window_ms / max(_time(f, 1), 1e-3))))
            t = {name: [] for name in runs}
            for _ in range(a.iters):                                            # alternating
                for name, f in runs.items():
                    t[name].append(_time(f, reps[name]))
            med = {name: sorted(v)[len(v) // 2] for name, v in t.items()}
            res = {k: ao(k, True) for k in sets}
            print(json.dumps(dict(input=kind, vox_res=S, radius_pitches=radius, samples_per_ray=M, texels=T, atlas=A,
                                  vertices=len(sets["vertices"]), atlas_texels=len(sets["atlas"]),
                                  ao_mean_vertices=round(float(res["vertices"].ao.mean()), 4), ao_mean_atlas=round(float(res["atlas"].ao.mean()), 4),
                                  open_share_vertices=round(float((res["vertices"].mask == -1).float().mean()), 4),
                                  skip_equals_noskip=same,
                                  **{name + "_ms": round(v, 4) for name, v in med.items()},
                                  **{name + "_ms_best": round(min(v), 4) for name, v in t.items()},
                                  atlas_ns_per_texel_skip=round(1e6 * med["ao_atlas_skip"] / max(1, len(sets["atlas"])), 3),
                                  atlas_ns_per_texel_noskip=round(1e6 * med["ao_atlas_noskip"] / max(1, len(sets["atlas"])), 3),
                                  reps=reps, iters=a.iters)), flush=True)


if __name__ == "__main__":
    main()
