"""Cost of the mesh statistics of `--eval.mesh_stats`: ops.mesh_topology (csrc/mesh_topology.hip: edge table, two union-finds, counts,
fixed-order float64 area and volume) at vox_res 64 and 128, B = 1, beside ops.isosurface_mesh on the same level grid -- a sphere and a
torus, sampled at lo + v (hi - lo) / (S - 1) as the evaluation does.  Device events around windows of `reps` calls (reps sized so that a
window is at least --window-ms long), after warm-up of every shape, the two ops alternating, in one process; medians and bests per
call.  Also the mesh's enclosed volume next to inside_voxels * pitch^3, the voxel count --eval.iou and --hip.largest_component work
with.  One JSON line per case.
python tools/perf_mesh_stats.py [--iters N] [--window-ms T] [--res 64,128] [--batches 1]"""
import argparse, json, os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch


def _time(f, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def level_grid(kind, B, S, lo, hi, dev):
    g = torch.linspace(lo, hi, S, device=dev, dtype=torch.float64)
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    if kind == "sphere":
        level = (x * x + y * y + z * z).sqrt() - 0.4
    else:                                                   # a torus of radii 0.3 and 0.12 around the z axis
        level = (((x * x + y * y).sqrt() - 0.3) ** 2 + z * z).sqrt() - 0.12
    return level.float()[None].expand(B, S, S, S).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--res", default="64,128")
    ap.add_argument("--batches", default="1")
    ap.add_argument("--range", default="-0.6,0.6")
    a = ap.parse_args()
    from shapeclipper_amd import ops
    dev = torch.device("cuda:0")
    lo, hi = (float(v) for v in a.range.split(","))
    for B in (int(x) for x in a.batches.split(",")):
        for kind in ("sphere", "torus"):
            for S in (int(v) for v in a.res.split(",")):
                level = level_grid(kind, B, S, lo, hi, dev)
                pitch = (hi - lo) / (S - 1)
                verts, faces, v_count, f_count = ops.isosurface_mesh(level)
                world = (lo + verts * pitch).contiguous()
                stats = ops.mesh_topology(world, faces, v_count, f_count)
                runs = {"mesh_topology": lambda: ops.mesh_topology(world, faces, v_count, f_count),
                        "isosurface_mesh": lambda: ops.isosurface_mesh(level)}
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
                inside = int((level[0] < 0).sum())
                print(json.dumps(dict(B=B, input=kind, vox_res=S, vertices=int(stats.vertices[0]), faces=int(stats.faces[0]),
                                      edges=int(stats.edges[0]), table_slots=ops.mesh_topology_slots(faces.shape[0]),
                                      watertight=bool(stats.watertight[0]), oriented=bool(stats.oriented[0]), manifold=bool(stats.manifold[0]),
                                      components=int(stats.components[0]), genus=int(stats.genus[0]), area=float(stats.area[0]),
                                      volume=float(stats.volume[0]), inside_voxels=inside, voxel_volume=inside * pitch ** 3,
                                      **{name + "_ms": round(v, 4) for name, v in med.items()},
                                      **{name + "_ms_best": round(min(v), 4) for name, v in t.items()},
                                      topology_over_mesher=round(med["mesh_topology"] / med["isosurface_mesh"], 2),
                                      reps=reps, iters=a.iters)), flush=True)


if __name__ == "__main__":
    main()
