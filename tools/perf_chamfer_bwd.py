"""Chamfer3D backward: the ordered kernels (csrc/chamfer_bwd.hip) against the atomic scatter (chamfer_grad_kernel) and the forward search of
the same clouds, at B = 1 and B = 32:
    uniform   N = M = 100,000 uniform clouds
    surface   the evaluation-like pair of tools/perf_chamfer_surface.py (spheres of radius 0.4 and 0.45, bumps 0.1)
    hub       50,000 sources that share one nearest neighbour (target 0 of 4,096; the others far away)
Event timing on the current stream, 3 warm-up calls, median of 15; the atomic figure includes the zero fill its contract needs.
Prints one JSON line.    python tools/perf_chamfer_bwd.py [--case NAME] [--batch B]      (one row, e.g. under rocprofv3 --kernel-trace --stats)
SHAPECLIPPER_HIP_LIB=<a build with -DSC_CHAMFER_BWD_CHUNK=n> measures another chunk length; "chunk" in the output says which."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chamfer_3D  # noqa: E402
from shapeclipper_amd import _lib, ops  # noqa: E402
from tools.perf_chamfer_surface import sphere  # noqa: E402

WARMUP, REPS = 3, 15


def clouds(case, B, gen):
    if case == "uniform":
        return torch.rand(B, 100000, 3, device="cuda", generator=gen) - 0.5, torch.rand(B, 100000, 3, device="cuda", generator=gen) - 0.5
    if case == "surface":
        return sphere(B, 100000, 0.4, gen), sphere(B, 100000, 0.45, gen, 0.1)
    a = (torch.rand(B, 50000, 3, device="cuda", generator=gen) - 0.5) * 0.02
    b = torch.rand(B, 4096, 3, device="cuda", generator=gen) + 5.0
    b[:, 0] = 0.0
    return a, b


def median_ms(fn):
    for _ in range(WARMUP):
        fn()
    times = []
    for _ in range(REPS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e))
    return round(statistics.median(times), 4)


def measure(case, B, gen):
    x1, x2 = clouds(case, B, gen)
    N, M = x1.shape[1], x2.shape[1]
    d1, d2 = torch.zeros(B, N, device="cuda"), torch.zeros(B, M, device="cuda")
    i1, i2 = torch.zeros(B, N, dtype=torch.int32, device="cuda"), torch.zeros(B, M, dtype=torch.int32, device="cuda")
    gd1, gd2 = torch.randn(B, N, device="cuda", generator=gen), torch.randn(B, M, device="cuda", generator=gen)
    g1, g2 = torch.zeros_like(x1), torch.zeros_like(x2)

    def atomic():
        g1.zero_(); g2.zero_()
        chamfer_3D.backward(x1, x2, g1, g2, gd1, gd2, i1, i2)

    row = dict(case=case, B=B, N=N, M=M)
    row["forward_ms"] = median_ms(lambda: chamfer_3D.forward(x1, x2, d1, d2, i1, i2))
    row["max_sources_per_row"] = int(max(torch.bincount(i1[0].long(), minlength=M).max(), torch.bincount(i2[0].long(), minlength=N).max()))
    row["ordered_ms"] = median_ms(lambda: ops.chamfer_backward_ordered(x1, x2, gd1, gd2, i1, i2))
    row["atomic_ms"] = median_ms(atomic)
    o1, o2 = ops.chamfer_backward_ordered(x1, x2, gd1, gd2, i1, i2)
    atomic()
    scale = max(float(g1.abs().max()), float(g2.abs().max()), 1e-30)
    row["max_abs_diff_over_max"] = max(float((o1 - g1).abs().max()), float((o2 - g2).abs().max())) / scale
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["uniform", "surface", "hub"])
    ap.add_argument("--batch", type=int)
    args = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = [measure(case, B, gen) for B in ([args.batch] if args.batch else [1, 32])
            for case in ([args.case] if args.case else ["uniform", "surface", "hub"])]
    print(json.dumps(dict(tool="perf_chamfer_bwd", device=torch.cuda.get_device_name(0), chunk=_lib.load().sc_chamfer3d_backward_ordered_chunk(),
                          warmup=WARMUP, reps=REPS, rows=rows)))


if __name__ == "__main__":
    main()
