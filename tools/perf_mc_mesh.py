"""Indexed marching-cubes mesh against the triangle soup on the evaluation's meshing workload (tools/perf_mc.py: 32 level grids at
vox_res = 100): ops.isosurface_mesh and ops.isosurface_triangles timed with device events, alternating, in one process.
python tools/perf_mc_mesh.py [--iters N]"""
import argparse, json, os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--images", type=int, default=32)
    a = ap.parse_args()
    from shapeclipper_amd import ops
    B, S = a.images, 101
    ax = torch.linspace(-0.6, 0.6, S, device="cuda")                 # the level grids of tools/workloads.py marching_cubes_100
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    gen = torch.Generator(device="cuda").manual_seed(0)
    r = 0.25 + 0.2 * torch.rand(B, 1, 1, 1, device="cuda", generator=gen)
    level = (torch.sqrt(X * X + Y * Y + 1.3 * Z * Z)[None] - r + 0.04 * torch.sin(9 * X)[None] * torch.cos(7 * Y)[None]).contiguous()
    runs = {"soup": lambda: ops.isosurface_triangles(level, 0.0), "mesh": lambda: ops.isosurface_mesh(level, 0.0)}
    for f in runs.values():                                            # warm-up: code objects, allocator
        f(); f()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(a.iters):                                           # alternate the two so drift hits both alike
        for k, f in runs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); f(); e.record()
            torch.cuda.synchronize()
            ms[k].append(s.elapsed_time(e))
    tris, per = runs["soup"]()
    verts, faces, vc, fc = runs["mesh"]()
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    print(json.dumps(dict(workload="marching cubes of %d level grids at vox_res=100" % B, triangles=int(per.sum()), vertices=int(vc.sum()),
                          soup_ms=round(med["soup"], 4), soup_ms_best=round(min(ms["soup"]), 4),
                          mesh_ms=round(med["mesh"], 4), mesh_ms_best=round(min(ms["mesh"]), 4),
                          ratio=round(med["mesh"] / med["soup"], 3), iters=a.iters,
                          note="each call includes its host read of the per-image counts (one synchronisation)")))


if __name__ == "__main__":
    main()
