"""Cost of the Earth Mover's Distance of `--eval.emd`: ops.emd_match (csrc/emd3d.hip, one workgroup per image) at n = 256, 1024 and 2048
points, B = 1 and B = 32, on two inputs -- uniform random clouds of [-0.5, 0.5]^3, and points on the sphere of radius 0.5 against uniform
points of the cube (mass that has to move: more rounds) -- against ONE chamfer_3D.forward on the same clouds.  Every image of a batch has
its own clouds.  Device events around windows of `reps` calls (reps sized so that a window is at least --window-ms long), after warm-up
of every shape, the two ops alternating, in one process; medians and bests per call, the rounds the auction took (min / mean / max over
the batch) and the time per round of the slowest image.  One JSON line per case.
python tools/perf_emd.py [--iters N] [--window-ms T] [--sizes 256,1024,2048] [--batches 1,32]"""
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
    gen.manual_seed(1000 * n + B)
    b = torch.rand(B, n, 3, device=dev, generator=gen) - 0.5
    if kind == "random":
        a = torch.rand(B, n, 3, device=dev, generator=gen) - 0.5
    else:
        d = torch.randn(B, n, 3, device=dev, generator=gen)
        a = 0.5 * d / d.norm(dim=-1, keepdim=True)
    return a.contiguous(), b.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--sizes", default="256,1024,2048")
    ap.add_argument("--batches", default="1,32")
    a = ap.parse_args()
    import chamfer_3D
    from shapeclipper_amd import ops
    dev = torch.device("cuda:0")
    for n in (int(x) for x in a.sizes.split(",")):
        for B in (int(x) for x in a.batches.split(",")):
            for kind in ("random", "sphere_cube"):
                x, y = clouds(kind, B, n, dev)
                d1, d2 = torch.zeros(B, n, device=dev), torch.zeros(B, n, device=dev)
                i1, i2 = torch.zeros(B, n, dtype=torch.int32, device=dev), torch.zeros(B, n, dtype=torch.int32, device=dev)
                runs = {"emd": lambda: ops.emd_match(x, y), "chamfer_forward": lambda: chamfer_3D.forward(x, y, d1, d2, i1, i2)}
                res = ops.emd_match(x, y)
                torch.cuda.synchronize()
                assert bool((res.converged == 1).all()), "the auction did not converge"
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
                rounds = res.rounds.double()
                print(json.dumps(dict(n=n, B=B, input=kind, emd_mean=round(float(res.emd.mean()), 6),
                                      rounds_min=int(rounds.min()), rounds_mean=round(float(rounds.mean()), 1), rounds_max=int(rounds.max()),
                                      **{name + "_ms": round(v, 4) for name, v in med.items()},
                                      **{name + "_ms_best": round(min(v), 4) for name, v in t.items()},
                                      us_per_round=round(1e3 * med["emd"] / float(rounds.max()), 3),
                                      emd_over_chamfer=round(med["emd"] / med["chamfer_forward"], 1),
                                      reps=reps, iters=a.iters)), flush=True)


if __name__ == "__main__":
    main()
