"""Cost and effect of the smoothing of `--mesh.smooth`: ops.mesh_smooth (csrc/mesh_smooth.hip: edge table, degree scan, sorted neighbour
rows, one launch per float64 half-step, chunked measures) at vox_res 64 and 128 for 1, 10 and 30 iterations at the default lam and mu,
B = 1, beside ops.isosurface_mesh and ops.mesh_topology on the same level grid -- a sphere and a torus, in grid-index units, as the
evaluation calls it.  Device events around windows of `reps` calls (reps sized so that a window is at least --window-ms long), after
warm-up of every shape, the three ops alternating, in one process; medians and bests per call (each call of the op ends with the host
read of its two flags, so the figure is the op as the evaluation pays for it).  Also the volume change, the roughness and the
displacement in object units (eval_3D.meshes_smoothed).  One JSON line per case.
python tools/perf_smooth.py [--iters N] [--window-ms T] [--res 64,128] [--smooth 1,10,30]"""
import argparse, json, os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch

from perf_mesh_stats import _time, level_grid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--res", default="64,128")
    ap.add_argument("--smooth", default="1,10,30")
    ap.add_argument("--range", default="-0.6,0.6")
    a = ap.parse_args()
    from shapeclipper_amd import ops
    from shapeclipper_amd.utils import eval_3D, options
    from shapeclipper_amd.utils.util import EasyDict as edict
    dev = torch.device("cuda:0")
    lo, hi = (float(v) for v in a.range.split(","))
    for kind in ("sphere", "torus"):
        for S in (int(v) for v in a.res.split(",")):
            level = level_grid(kind, 1, S, lo, hi, dev)
            packed = ops.isosurface_mesh(level)
            for n in (int(v) for v in a.smooth.split(",")):
                opt = edict(eval=dict(range=[lo, hi]), mesh=dict(smooth=n))
                _, lam, mu = options.smooth_settings(opt)
                var = edict(level_vox=level, mesh_packed=list(packed))
                eval_3D.meshes_smoothed(opt, var)
                res = var.mesh_smoothed
                runs = {"mesh_smooth": lambda: ops.mesh_smooth(*packed, n, lam, mu),
                        "isosurface_mesh": lambda: ops.isosurface_mesh(level),
                        "mesh_topology": lambda: ops.mesh_topology(*packed)}
                reps = {}
                for name, f in runs.items():                                    # warm-up, then the size of a window
                    f(); f()
                    torch.cuda.synchronize()
                    reps[name] = max(1, min(1000, int(a.window_ms / max(_time(f, 1), 1e-3))))
                t = {name: [] for name in runs}
                for _ in range(a.iters):                                        # alternating
                    for name, f in runs.items():
                        t[name].append(_time(f, reps[name]))
                med = {name: sorted(v)[len(v) // 2] for name, v in t.items()}
                one = lambda key: float(res[key][0])
                print(json.dumps(dict(input=kind, vox_res=S, smooth=n, lam=lam, mu=round(mu, 6), launches=7 + 2 * n,
                                      vertices=int(packed[2][0]), faces=int(packed[3][0]),
                                      free=int(res["free"][0]), fixed_boundary=int(res["fixed_boundary"][0]), degree_max=int(res["degree_max"][0]),
                                      volume_change=round(one("volume_after") / one("volume_before") - 1.0, 6),
                                      area_change=round(one("area_after") / one("area_before") - 1.0, 6),
                                      rough_before=one("rough_before"), rough_after=one("rough_after"), disp_mean=one("disp_mean"),
                                      disp_max=one("disp_max"), grid_pitch=(hi - lo) / (S - 1),
                                      **{name + "_ms": round(v, 4) for name, v in med.items()},
                                      **{name + "_ms_best": round(min(v), 4) for name, v in t.items()},
                                      smooth_over_mesher=round(med["mesh_smooth"] / med["isosurface_mesh"], 2),
                                      us_per_launch=round(1000.0 * med["mesh_smooth"] / (7 + 2 * n), 2),
                                      reps=reps, iters=a.iters)), flush=True)


if __name__ == "__main__":
    main()
