"""Cost and effect of `--mesh.decimate`: ops.mesh_decimate (csrc/mesh_decimate.hip: 14 launches and one host read a round, rounds until the
face budget is met) going to 1/2, 1/4 and 1/10 of the faces, B = 1, beside ops.mesh_cluster_simplify (cells of 2 and 4 grid pitches),
ops.mesh_topology and ops.isosurface_mesh on the same mesh -- a geometric-init SDF network (roughly a sphere of radius 0.5, zero latent)
at vox_res 64 and 128.  Device events around windows of `reps` calls (reps sized so that a window is at least --window-ms long; one
call for the decimations), after warm-up, the runs alternating, in one process; medians and bests per call (every round of the op ends
with its host read, so the figure is the op as the evaluation pays for it).  Per budget also the rounds, the time per round, the faces
reached and the mean and largest distance from the original vertices to the result, in grid pitches, beside clustering's.
One JSON line per resolution.
python tools/perf_decimate.py [--iters N] [--window-ms T] [--res 64,128]"""
import argparse, json, os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch

from perf_mesh_stats import _time
from perf_subdivide import _measure


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--res", default="64,128")
    a = ap.parse_args()
    from shapeclipper_amd import ops
    from shapeclipper_amd.model.implicit import SDFNetwork
    from shapeclipper_amd.utils import eval_3D, options
    from shapeclipper_amd.utils.util import EasyDict as edict
    dev = torch.device("cuda:0")
    opt = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=perf_decimate",
                                               "--output_root=/tmp/sc_perf"]), verbose=False)
    torch.manual_seed(0)
    sdf_net = SDFNetwork(opt).to(dev)
    zs = torch.zeros(1, opt.arch.impl_sdf.proj_latent_dim, device=dev)
    for vox in (int(v) for v in a.res.split(",")):
        opt.eval.vox_res = vox
        with torch.no_grad():
            var = edict(idx=torch.arange(1, device=dev), proj_latent_sdf=zs)
            level = eval_3D.compute_level_grid(opt, sdf_net, zs, eval_3D.get_dense_3D_grid(opt, var))
            S = level.shape[1]
            packed = ops.isosurface_mesh(level)
            F = int(packed.f_count[0])
            budgets = {"1/2": F // 2, "1/4": F // 4, "1/10": F // 10}
            cells = {k: -(-(S - 1) // k) for k in (2, 4)}
            runs = {"isosurface_mesh": lambda: ops.isosurface_mesh(level),
                    "mesh_topology": lambda: ops.mesh_topology(*packed),
                    "cluster_2": lambda: ops.mesh_cluster_simplify(*packed, (0.0, 0.0, 0.0), 2.0, cells[2]),
                    "cluster_4": lambda: ops.mesh_cluster_simplify(*packed, (0.0, 0.0, 0.0), 4.0, cells[4])}
            med, best, reps = _measure(runs, a.iters, a.window_ms)

            def far(mesh):
                d = ops.point_mesh_distance(packed.verts[None].contiguous(), *mesh.packed).dist2.sqrt()[0]
                return round(float(d.mean()), 6), round(float(d.max()), 6)

            out = dict(vox_res=vox, vertices=int(packed.v_count[0]), faces=F, **{k + "_ms": round(v, 4) for k, v in med.items()},
                       **{k + "_ms_best": round(v, 4) for k, v in best.items()}, reps=reps, iters=a.iters)
            for k in (2, 4):
                c = runs["cluster_%d" % k]()
                out["cluster_%d_faces" % k] = int(c.f_count[0])
                out["cluster_%d_dist_mean" % k], out["cluster_%d_dist_max" % k] = far(c)
            for name, target in budgets.items():
                f = lambda: ops.mesh_decimate(*packed, target)
                res = f()
                torch.cuda.synchronize()
                t = sorted(_time(f, 1) for _ in range(a.iters))
                topo = ops.mesh_topology(*res.packed)
                mean, top = far(res)
                n = int(res.rounds[0])
                out["decimate_" + name] = dict(target=target, faces=int(res.f_count[0]), vertices=int(res.v_count[0]), rounds=n,
                                               collapses=int(res.collapses[0]), rejected_link=int(res.rejected_link[0]),
                                               rejected_flip=int(res.rejected_flip[0]), reached=int(res.reached[0]),
                                               ms=round(t[len(t) // 2], 3), ms_best=round(t[0], 3), ms_per_round=round(t[len(t) // 2] / max(n, 1), 4),
                                               dist_mean=mean, dist_max=top, watertight=bool(topo.watertight[0]), manifold=bool(topo.manifold[0]),
                                               genus=int(topo.genus[0]))
            print(json.dumps(out), flush=True)
            del level
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
