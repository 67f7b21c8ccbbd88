"""Cost and effect of the decimation of `--eval.simplify`: ops.mesh_cluster_simplify (csrc/mesh_simplify.hip: cell mask and rank scan,
int64 quadric accumulators fed by 64-bit atomics, per-cluster float64 solve, parity table, block-scan compaction) at vox_res 64 and 128
for k = 2 and 4, B = 1, beside ops.isosurface_mesh and ops.mesh_topology on the same level grid -- a sphere and a torus, in grid-index
units with origin 0, as the evaluation calls it.  Device events around windows of `reps` calls (reps sized so that a window is at least
--window-ms long), after warm-up of every shape, the three ops alternating, in one process; medians and bests per call (each call of the
op ends with the host read that sizes its outputs, so the figure is the op as the evaluation pays for it).  Also the face ratio, the
topology of the simplified mesh and the distance of the original vertices to it in object units (eval_3D.meshes_simplified).  One JSON
line per case.
python tools/perf_simplify.py [--iters N] [--window-ms T] [--res 64,128] [--cells 2,4]"""
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
    ap.add_argument("--cells", default="2,4")
    ap.add_argument("--range", default="-0.6,0.6")
    a = ap.parse_args()
    from shapeclipper_amd import ops
    from shapeclipper_amd.utils import eval_3D
    from shapeclipper_amd.utils.util import EasyDict as edict
    dev = torch.device("cuda:0")
    lo, hi = (float(v) for v in a.range.split(","))
    for kind in ("sphere", "torus"):
        for S in (int(v) for v in a.res.split(",")):
            level = level_grid(kind, 1, S, lo, hi, dev)
            packed = ops.isosurface_mesh(level)
            for k in (int(v) for v in a.cells.split(",")):
                G = -(-(S - 1) // k)
                var = edict(level_vox=level, mesh_packed=list(packed))
                eval_3D.meshes_simplified(edict(eval=dict(range=[lo, hi], simplify=k, mesh_stats=True)), var)
                res, stats = var.mesh_simplified, var.mesh_stats_simplified
                runs = {"mesh_cluster_simplify": lambda: ops.mesh_cluster_simplify(*packed, (0.0, 0.0, 0.0), float(k), G, 0.05),
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
                f_in, f_out = int(packed[3][0]), int(res["f_count"][0])
                print(json.dumps(dict(input=kind, vox_res=S, cell=k, cells_per_axis=G, vertices_in=int(packed[2][0]), faces_in=f_in,
                                      vertices_out=int(res["v_count"][0]), faces_out=f_out, face_ratio=round(f_out / max(f_in, 1), 4),
                                      collapsed=int(res["collapsed"][0]), cancelled=int(res["cancelled"][0]),
                                      dist_mean=float(res["dist_mean"][0]), dist_max=float(res["dist_max"][0]),
                                      grid_pitch=(hi - lo) / (S - 1), watertight=bool(stats["watertight"][0]),
                                      manifold=bool(stats["manifold"][0]), oriented=bool(stats["oriented"][0]), genus=int(stats["genus"][0]),
                                      unreferenced=int(stats["unreferenced_vertices"][0]),
                                      **{name + "_ms": round(v, 4) for name, v in med.items()},
                                      **{name + "_ms_best": round(min(v), 4) for name, v in t.items()},
                                      simplify_over_mesher=round(med["mesh_cluster_simplify"] / med["isosurface_mesh"], 2),
                                      reps=reps, iters=a.iters)), flush=True)


if __name__ == "__main__":
    main()
