#!/usr/bin/env python
"""Cost of the turn-table of training-time visualisation (`--hip.train_vis`): 3 samples x 50 views x 64^2 rays x 64 samples on one GPU.

    python tools/perf_turntable.py [--iters 5]

  per_view          Runner.vis_rotate(batched=False) per sample: the reference's loop, 3 x 50 renders of 4,096 rays
  batched           Runner.vis_rotate(batched=True) per sample, as Runner.visualize_samples calls it: 3 passes of 204,800 rays
  batched_together  the 3 samples in one call: 2 passes of 307,200 rays (at most 524,288 rays per pass)
  frames            the three ops.vis_frames launches of the 3 samples' GIF frames

Each figure is the median wall time of `iters` runs that end in a device synchronise, the CPU-generator draws included (the
reference's, made by both forms).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    from shapeclipper_amd.model.graph import Graph
    from shapeclipper_amd.model.implicit import RGBNetwork, SDFNetwork
    from shapeclipper_amd.model.renderer import Renderer
    from shapeclipper_amd.model.runner import Runner
    from shapeclipper_amd.utils import camera, options
    from shapeclipper_amd.utils.util import EasyDict as edict

    dev = torch.device("cuda")
    opt = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=perf_turntable",
                                               "--output_root=/tmp/sc_perf"]), verbose=False)
    opt.H, opt.W = opt.eval.image_size
    torch.manual_seed(0)
    sdf_net, rgb_net = SDFNetwork(opt), RGBNetwork(opt)
    runner = types.SimpleNamespace(graph=types.SimpleNamespace(module=types.SimpleNamespace(renderer=Renderer(opt, sdf_net, rgb_net).to(dev))))
    N, V = 3, 50

    def sample(b):
        var = edict(idx=torch.arange(b, device=dev), intr=camera.get_intr(opt, torch.ones(b)).to(dev), scale_dist=torch.ones(b, device=dev),
                    proj_latent_sdf=torch.randn(b, 64, device=dev), proj_latent_rgb=torch.randn(b, 64, device=dev),
                    rgb_input_map=torch.zeros(b, 3, 2, 2, device=dev))
        return Graph.get_rotate_pose(None, opt, var, n_views=V)
    singles, together = [sample(1) for _ in range(N)], sample(N)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.iters):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) * 1e3)
        return round(float(np.median(ts)), 3), round(min(ts), 3), round(max(ts), 3)

    rot = lambda var, batched: Runner.vis_rotate(runner, opt, var, n_views=V, batched=batched)
    res = dict(samples=N, views=V, H=opt.H, W=opt.W, n_samples=opt.render.n_samples_uniform, iters=args.iters)
    for name, fn in (("per_view", lambda: [rot(v, False) for v in singles]), ("batched", lambda: [rot(v, True) for v in singles]),
                     ("batched_together", lambda: rot(together, True)),
                     ("frames", lambda: [Runner.turntable_frames(opt, v) for v in singles])):
        med, lo, hi = timed(fn)
        res.update({name + "_ms": med, name + "_ms_min": lo, name + "_ms_max": hi})
    res["speedup_batched"] = round(res["per_view_ms"] / res["batched_ms"], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
