"""Cost of the mesh-based completeness of `--eval.mesh_dist`: the exact grid search of csrc/point_mesh.hip against its all-pairs twin and
against ONE chamfer_3D.forward, at the evaluation's shape -- B = 1, 100,000 ground-truth points against the marching-cubes mesh of a
sphere on the evaluation's level grid (eval.vox_res = 64 by default, --vox to change), the points on a concentric sphere `--offset`
away from the mesh (0.03 of the unit range: a few cells of the search grid), and the same points against 100,000 samples of the
mesh for Chamfer.  The two searches are timed through the C ABI (outputs and workspace allocated once; ops.point_mesh_distance adds the
validation reduction and its one host read, timed as `op`), with device events after warm-up, alternating, in one process; medians
and bests.  The grid search and the twin must agree bit for bit, which is checked before anything is timed.
python tools/perf_point_mesh.py [--iters N] [--points P] [--vox S] [--offset D]"""
import argparse, json, os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch


def _time(f):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(); f(); e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--brute-iters", type=int, default=3)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--vox", type=int, default=64)
    ap.add_argument("--offset", type=float, default=0.03)
    a = ap.parse_args()
    import chamfer_3D
    from shapeclipper_amd import _lib, ops
    from shapeclipper_amd.utils import eval_3D
    dev = torch.device("cuda:0")
    lo, hi, radius = -0.6, 0.6, 0.4
    g = torch.linspace(lo, hi, a.vox + 1, device=dev)
    level = (torch.stack(torch.meshgrid(g, g, g, indexing="ij"), dim=-1).norm(dim=-1) - radius)[None].contiguous()
    (verts, faces), = eval_3D.meshes_device(level, lo, hi)
    verts, faces = verts.contiguous(), faces.contiguous()
    samples, _ = eval_3D.surface_points_device(level, lo, hi, a.points, seed=0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    d = torch.randn(1, a.points, 3, device=dev, generator=gen)
    centre = samples.mean(dim=1, keepdim=True)                   # the written mesh carries the v / S rescale: it is not centred at 0
    pts = (centre + (radius * a.vox / (a.vox + 1) + a.offset) * d / d.norm(dim=-1, keepdim=True)).contiguous()
    V, F, P = verts.shape[0], faces.shape[0], a.points
    i32 = dict(dtype=torch.int32, device=dev)
    v_count, f_count = torch.tensor([V], **i32), torch.tensor([F], **i32)
    lib = _lib.load()
    ws = torch.empty((int(lib.sc_point_mesh_workspace_bytes(1, P, V, F)) + 3) // 4, device=dev)
    out = {k: (torch.empty(1, P, device=dev), torch.empty(1, P, **i32), torch.empty(1, P, 3, device=dev)) for k in ("grid", "brute")}
    p = _lib.ptr

    def raw(kind):
        fn = lib.sc_point_mesh_distance if kind == "grid" else lib.sc_point_mesh_distance_brute
        d2, f, q = out[kind]
        _lib.check(fn(p(pts), p(verts), p(faces), p(v_count), p(f_count), 1, P, V, F, p(ws), p(d2), p(f), p(q), _lib.stream()), kind)

    d1, d2 = torch.zeros(1, P, device=dev), torch.zeros(1, P, device=dev)
    i1, i2 = torch.zeros(1, P, **i32), torch.zeros(1, P, **i32)
    runs = {"grid": lambda: raw("grid"), "op": lambda: ops.point_mesh_distance(pts, verts, faces, v_count, f_count),
            "chamfer_forward": lambda: chamfer_3D.forward(samples, pts, d1, d2, i1, i2)}
    raw("grid"); raw("brute")
    torch.cuda.synchronize()
    for x, y in zip(out["grid"], out["brute"]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "grid and brute differ"
    for f in runs.values():                                                                 # warm-up: code objects, allocator, scratch
        f(); f()
    torch.cuda.synchronize()
    res = {name: [] for name in runs}
    for _ in range(a.iters):                                                                # alternating
        for name, f in runs.items():
            res[name].append(_time(f))
    res["brute"] = [_time(lambda: raw("brute")) for _ in range(a.brute_iters)]
    med = {name: sorted(v)[len(v) // 2] for name, v in res.items()}
    dist = out["grid"][0].sqrt()
    print(json.dumps(dict(points=P, vox=a.vox, verts=V, faces=F, offset=a.offset, mean_distance=round(float(dist.mean()), 5),
                          chamfer_search=chamfer_3D._path(P, P), workspace_mb=round(ws.numel() * 4 / 2 ** 20, 1),
                          **{name + "_ms": round(v, 4) for name, v in med.items()},
                          **{name + "_ms_best": round(min(v), 4) for name, v in res.items()},
                          grid_over_chamfer=round(med["grid"] / med["chamfer_forward"], 3),
                          brute_over_grid=round(med["brute"] / med["grid"], 2), iters=a.iters, brute_iters=a.brute_iters)), flush=True)


if __name__ == "__main__":
    main()
