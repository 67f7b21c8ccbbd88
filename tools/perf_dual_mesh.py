"""Dual-contouring mesh cost: ops.dual_contour_mesh against ops.isosurface_mesh alone on the same grids, timed with device events after
warm-up, alternating, in one process.  32 level grids of 101^3 (eval.vox_res = 100): spheres of different radii and centres, with their
analytic unit normals at the crossing vertices, so no network is involved.  dual_contour_mesh repeats isosurface_mesh's count, scan and
vertex emit, so `dual_over_mesh_ms` is the price of the dual passes themselves minus the marching-cubes face emit.
python tools/perf_dual_mesh.py [--iters N] [--images B] [--side S]"""
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--side", type=int, default=101)
    a = ap.parse_args()
    from shapeclipper_amd import ops
    dev = torch.device("cuda:0")
    B, S = a.images, a.side
    g = torch.arange(S, device=dev, dtype=torch.float32)
    pts = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), dim=-1)                       # grid-index units
    k = torch.arange(B, device=dev, dtype=torch.float32)
    centre = (S - 1) / 2 + torch.stack([0.05 * k, -0.03 * k, 0.02 * k], 1) * (S - 1) / 2    # [B,3]
    radius = (0.3 + 0.5 * k / max(B - 1, 1)) * (S - 1) / 2
    level = ((pts[None] - centre[:, None, None, None]).norm(dim=-1) - radius[:, None, None, None]).contiguous()
    verts, faces, vc, fc = ops.isosurface_mesh(level)
    image = torch.repeat_interleave(torch.arange(B, device=dev), vc.to(dev))
    normals = torch.nn.functional.normalize(verts - centre[image], dim=1).contiguous()
    runs = {"isosurface_mesh": lambda: ops.isosurface_mesh(level), "dual_contour_mesh": lambda: ops.dual_contour_mesh(level, normals)}
    for f in runs.values():                                                                 # warm-up: code objects, allocator, scratch
        f(); f()
    torch.cuda.synchronize()
    res = {name: [] for name in runs}
    for _ in range(a.iters):                                                                # alternating
        for name, f in runs.items():
            res[name].append(_time(f, 1)[0])
    med = {name: sorted(v)[len(v) // 2] for name, v in res.items()}
    dv, df, dvc, dfc = ops.dual_contour_mesh(level, normals)
    print(json.dumps(dict(images=B, side=S, mc_vertices=int(vc.sum()), mc_faces=int(fc.sum()), dual_vertices=int(dvc.sum()),
                          dual_faces=int(dfc.sum()), **{name + "_ms": round(v, 4) for name, v in med.items()},
                          **{name + "_ms_best": round(min(v), 4) for name, v in res.items()},
                          dual_over_mesh_ms=round(med["dual_contour_mesh"] - med["isosurface_mesh"], 4), iters=a.iters)), flush=True)


if __name__ == "__main__":
    main()
