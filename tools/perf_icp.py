"""Cost of the evaluation's ICP: ops.icp_align (30 rounds by default) against ONE chamfer_3D.forward on the same clouds, 100k x 100k points,
B = 1 and B = 32, timed with device events after warm-up, alternating, in one process; medians.  The clouds are two noisy samplings of
a box surface, the target moved by a small similarity, so the search sees what the evaluation gives it.  `per_round_ms` is
icp_align / (iters + 1): apply + two-direction search + objective + fit; `round_over_search` says how much of a round is not the search.
python tools/perf_icp.py [--iters N] [--points P] [--rounds R] [--images 1 32]"""
import argparse, json, math, os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch


def _time(f):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(); f(); e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def _clouds(B, P, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    half = torch.tensor([0.3, 0.2, 0.25], device=dev)

    def surface():
        p = (torch.rand(B, P, 3, device=dev, generator=g) * 2 - 1) * half
        axis = torch.randint(0, 3, (B, P, 1), device=dev, generator=g)
        side = (torch.randint(0, 2, (B, P, 1), device=dev, generator=g) * 2 - 1).float()
        return p.scatter(2, axis, side * half[axis.squeeze(-1)].unsqueeze(-1))
    src, dst = surface(), surface()
    a = math.radians(8.0)
    R = torch.tensor([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]], device=dev)
    dst = 1.05 * dst @ R.T + torch.tensor([0.02, -0.01, 0.03], device=dev)
    return src.contiguous(), dst.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10, help="timed repetitions of each of the two calls")
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=30, help="icp_align's iters")
    ap.add_argument("--images", type=int, nargs="+", default=[1, 32])
    a = ap.parse_args()
    import chamfer_3D
    from shapeclipper_amd import ops
    dev = torch.device("cuda:0")
    for B in a.images:
        P = a.points
        src, dst = _clouds(B, P, dev)
        d1, d2 = torch.zeros(B, P, device=dev), torch.zeros(B, P, device=dev)
        i1, i2 = torch.zeros(B, P, dtype=torch.int32, device=dev), torch.zeros(B, P, dtype=torch.int32, device=dev)
        runs = {"chamfer_forward": lambda: chamfer_3D.forward(src, dst, d1, d2, i1, i2),
                "icp_align": lambda: ops.icp_align(src, dst, iters=a.rounds)}
        for f in runs.values():                                                             # warm-up: code objects, allocator, scratch
            f(); f()
        torch.cuda.synchronize()
        res = {name: [] for name in runs}
        for _ in range(a.iters):                                                            # alternating
            for name, f in runs.items():
                res[name].append(_time(f))
        med = {name: sorted(v)[len(v) // 2] for name, v in res.items()}
        out = ops.icp_align(src, dst, iters=a.rounds)
        per_round = med["icp_align"] / (a.rounds + 1)
        print(json.dumps(dict(images=B, points=P, rounds=a.rounds, search=chamfer_3D._path(P, P),
                              **{name + "_ms": round(v, 4) for name, v in med.items()},
                              **{name + "_ms_best": round(min(v), 4) for name, v in res.items()},
                              per_round_ms=round(per_round, 4), round_over_search=round(per_round / med["chamfer_forward"], 3),
                              objective_first=float(out.objective[0, 0]), objective_last=float(out.objective[0, -1]),
                              s=float(out.s[0]), iters=a.iters)), flush=True)


if __name__ == "__main__":
    main()
