"""Cost of the ground-truth normals of `--eval.normals`: ops.knn_points + ops.point_normals at B = 1, N = 100,000, k = 16 on a sphere
surface and on a uniform volume, against ONE chamfer_3D.forward of the same sizes (the cloud against a second sampling of the same
shape), timed with device events after warm-up, alternating, in one process; medians and bests.
`--scan` times the all-points scan instead (SC_KNN_FORCE_SCAN=1 must be in the environment before the library is first called: the
switch is read once) -- run it as a second process and with few iterations, a scan of 100,000 x 100,000 keys takes a while.
python tools/perf_normals.py [--iters N] [--points P] [--k K] [--scan]"""
import argparse, json, os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch


def _time(f):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(); f(); e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def _cloud(kind, P, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    if kind == "volume":
        return (torch.rand(1, P, 3, device=dev, generator=g) - 0.5).contiguous()
    v = torch.randn(1, P, 3, device=dev, generator=g)
    return (0.5 * v / v.norm(dim=-1, keepdim=True)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--scan", action="store_true", help="the forced all-points scan (needs SC_KNN_FORCE_SCAN=1 in the environment)")
    a = ap.parse_args()
    if a.scan and os.environ.get("SC_KNN_FORCE_SCAN") != "1":
        sys.exit("perf_normals.py --scan: set SC_KNN_FORCE_SCAN=1 in the environment")
    if not a.scan and os.environ.get("SC_KNN_FORCE_SCAN", "0") != "0":
        sys.exit("perf_normals.py: SC_KNN_FORCE_SCAN is set; pass --scan to time the scan")
    import chamfer_3D
    from shapeclipper_amd import ops
    dev = torch.device("cuda:0")
    P, k = a.points, a.k
    for kind in ("sphere", "volume"):
        pts, other = _cloud(kind, P, dev, 0), _cloud(kind, P, dev, 1)
        d1, d2 = torch.zeros(1, P, device=dev), torch.zeros(1, P, device=dev)
        i1, i2 = torch.zeros(1, P, dtype=torch.int32, device=dev), torch.zeros(1, P, dtype=torch.int32, device=dev)
        idx, _ = ops.knn_points(pts, k)
        runs = {"knn_points": lambda: ops.knn_points(pts, k),
                "point_normals_given_idx": lambda: ops.point_normals(pts, k, idx=idx),
                "chamfer_forward": lambda: chamfer_3D.forward(pts, other, d1, d2, i1, i2)}
        for f in runs.values():                                                             # warm-up: code objects, allocator, scratch
            f(); f()
        torch.cuda.synchronize()
        res = {name: [] for name in runs}
        for _ in range(a.iters):                                                            # alternating
            for name, f in runs.items():
                res[name].append(_time(f))
        med = {name: sorted(v)[len(v) // 2] for name, v in res.items()}
        normals = ops.point_normals(pts, k, idx=idx)
        print(json.dumps(dict(cloud=kind, points=P, k=k, scan=bool(a.scan), search=chamfer_3D._path(P, P),
                              **{name + "_ms": round(v, 4) for name, v in med.items()},
                              **{name + "_ms_best": round(min(v), 4) for name, v in res.items()},
                              knn_plus_normals_ms=round(med["knn_points"] + med["point_normals_given_idx"], 4),
                              knn_over_chamfer=round(med["knn_points"] / med["chamfer_forward"], 3),
                              degenerate_points=int((normals.variation == 0).sum()), iters=a.iters)), flush=True)


if __name__ == "__main__":
    main()
