"""Cost of the check of `--mesh.self_intersect`: ops.mesh_self_intersections (csrc/mesh_intersect.hip) with search="grid" -- the triangle
grid of csrc/triangle_grid.hpp, every candidate pair tested once by a filtered float64 sign rule -- beside its all-pairs twin
search="brute" and ops.mesh_topology on the same meshes, B = 1: the marching-cubes mesh of a geometric-init SDF network (roughly a sphere
of radius 0.5, zero latent) at vox_res 64 and 128, and its one-level Loop subdivision (four times the faces).  Device events around
windows of `reps` calls (reps sized so that a window is at least --window-ms long), after warm-up, the runs alternating, in one process;
medians and bests per call, the op's one host read (its two flags) included.  The all-pairs twin is quadratic in the faces: it is
skipped above --brute-max-faces (default 150,000) and the line says so.  One JSON line per mesh, with the op's counts.
python tools/perf_self_intersect.py [--iters N] [--window-ms T] [--res 64,128] [--brute-max-faces F]"""
import argparse, json, os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch

from perf_subdivide import _measure


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--res", default="64,128")
    ap.add_argument("--brute-max-faces", type=int, default=150000)
    a = ap.parse_args()
    from shapeclipper_amd import ops
    from shapeclipper_amd.model.implicit import SDFNetwork
    from shapeclipper_amd.utils import eval_3D, options
    from shapeclipper_amd.utils.util import EasyDict as edict
    dev = torch.device("cuda:0")
    opt = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=perf_self_intersect",
                                               "--output_root=/tmp/sc_perf"]), verbose=False)
    torch.manual_seed(0)
    sdf_net = SDFNetwork(opt).to(dev)
    zs = torch.zeros(1, opt.arch.impl_sdf.proj_latent_dim, device=dev)
    for vox in (int(v) for v in a.res.split(",")):
        opt.eval.vox_res = vox
        with torch.no_grad():
            var = edict(idx=torch.arange(1, device=dev), proj_latent_sdf=zs)
            level = eval_3D.compute_level_grid(opt, sdf_net, zs, eval_3D.get_dense_3D_grid(opt, var))
            plain = ops.isosurface_mesh(level)
            meshes = {"mc": plain, "subdiv": ops.mesh_subdivide(*plain, 1).packed}
            for name, mesh in meshes.items():
                F = int(mesh.f_count[0])
                runs = {"self_intersections_grid": lambda: ops.mesh_self_intersections(*mesh, search="grid"),
                        "mesh_topology": lambda: ops.mesh_topology(*mesh)}
                if F <= a.brute_max_faces:
                    runs["self_intersections_brute"] = lambda: ops.mesh_self_intersections(*mesh, search="brute")
                med, best, reps = _measure(runs, a.iters, a.window_ms)
                res = ops.mesh_self_intersections(*mesh, search="grid")
                print(json.dumps(dict(vox_res=vox, mesh=name, vertices=int(mesh.v_count[0]), faces=F, pairs=int(res.pairs[0]),
                                      pairs_vertex=int(res.pairs_vertex[0]), box_pairs=int(res.box_pairs[0]), faces_hit=int(res.faces_hit[0]),
                                      degenerate=int(res.degenerate[0]), brute_skipped=F > a.brute_max_faces,
                                      **{k + "_ms": round(v, 4) for k, v in med.items()},
                                      **{k + "_ms_best": round(v, 4) for k, v in best.items()},
                                      ns_per_face_grid=round(med["self_intersections_grid"] * 1e6 / max(F, 1), 2), reps=reps, iters=a.iters)),
                      flush=True)
            del level
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
