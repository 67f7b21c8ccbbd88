"""Cost of the volumetric IoU of `--eval.iou`: ops.voxel_frame + two ops.voxel_solid (csrc/voxel_solid.hip, one workgroup per cloud) +
ops.voxel_iou at N = 100,000 points a cloud, B = 1, R = 32 and 64, close = 0, 1 and 2, on two inputs -- points on the sphere of radius
0.5 against a scaled, moved copy, and the sphere against the surface of a box -- against ONE chamfer_3D.forward on the same clouds.
Device events around windows of `reps` calls (reps sized so that a window is at least --window-ms long), after warm-up of every shape,
the two ops alternating, in one process; medians and bests per call, the split of the IoU into its three entry points, and the sweeps
of the exterior flood of the two solids.  One JSON line per case.
python tools/perf_iou.py [--iters N] [--window-ms T] [--points 100000] [--res 32,64] [--close 0,1,2] [--batches 1]"""
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


def clouds(kind, B, n, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000 + B)
    d = torch.randn(B, n, 3, device=dev, generator=gen)
    a = 0.5 * d / d.norm(dim=-1, keepdim=True)
    if kind == "sphere_copy":
        b = 1.05 * a.flip(1) + 0.02
    else:                                                   # the surface of the box of half extents 0.45, 0.4, 0.3: a face, a point on it
        u = torch.rand(B, n, 3, device=dev, generator=gen) * 2 - 1
        axis = torch.randint(0, 3, (B, n, 1), device=dev, generator=gen)
        b = u.scatter(2, axis, torch.sign(u.gather(2, axis)) + (u.gather(2, axis) == 0)) * torch.tensor([0.45, 0.4, 0.3], device=dev)
    return a.contiguous(), b.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--res", default="32,64")
    ap.add_argument("--close", default="0,1,2")
    ap.add_argument("--batches", default="1")
    a = ap.parse_args()
    import chamfer_3D
    from shapeclipper_amd import ops
    dev = torch.device("cuda:0")
    n = a.points
    for B in (int(x) for x in a.batches.split(",")):
        for kind in ("sphere_copy", "sphere_box"):
            x, y = clouds(kind, B, n, dev)
            d1, d2 = torch.zeros(B, n, device=dev), torch.zeros(B, n, device=dev)
            i1, i2 = torch.zeros(B, n, dtype=torch.int32, device=dev), torch.zeros(B, n, dtype=torch.int32, device=dev)
            for res in (int(v) for v in a.res.split(",")):
                for close in (int(v) for v in a.close.split(",")):
                    origin, pitch = ops.voxel_frame(x, y, res, close)
                    sx, sy = ops.voxel_solid(x, origin, pitch, res, close), ops.voxel_solid(y, origin, pitch, res, close)
                    inter, union = ops.voxel_iou(sx.bits, sy.bits)

                    def iou():
                        o, p = ops.voxel_frame(x, y, res, close)
                        return ops.voxel_iou(ops.voxel_solid(x, o, p, res, close).bits, ops.voxel_solid(y, o, p, res, close).bits)
                    runs = {"iou": iou, "frame": lambda: ops.voxel_frame(x, y, res, close),
                            "solid": lambda: ops.voxel_solid(x, origin, pitch, res, close),
                            "popcount": lambda: ops.voxel_iou(sx.bits, sy.bits),
                            "chamfer_forward": lambda: chamfer_3D.forward(x, y, d1, d2, i1, i2)}
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
                    print(json.dumps(dict(n=n, B=B, input=kind, res=res, close=close,
                                          iou=round(float((inter.double() / union.double().clamp(min=1)).mean()), 6),
                                          shell=[int(sx.shell_voxels.max()), int(sy.shell_voxels.max())],
                                          solid=[int(sx.solid_voxels.max()), int(sy.solid_voxels.max())],
                                          sweeps=[int(sx.sweeps.max()), int(sy.sweeps.max())],
                                          **{name + "_ms": round(v, 4) for name, v in med.items()},
                                          **{name + "_ms_best": round(min(v), 4) for name, v in t.items()},
                                          iou_over_chamfer=round(med["iou"] / med["chamfer_forward"], 2),
                                          reps=reps, iters=a.iters)), flush=True)


if __name__ == "__main__":
    main()
