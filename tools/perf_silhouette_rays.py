#!/usr/bin/env python
"""Cost of the Pix3D loader's silhouette ray choice.

    python tools/perf_silhouette_rays.py device    # (a) ops.silhouette_distance + ops.silhouette_rays, 192 masks of 224x224 (GPU)
    python tools/perf_silhouette_rays.py host      # (b) utils.util.compute_sampling_prob per 224x224 mask (CPU)
    python tools/perf_silhouette_rays.py loader    # (c) loader samples/s on a generated 224x224 tree, num_workers 16,
                                                   #     hip.device_rays on and off (never opens the GPU: the workers are forked)
    python tools/perf_silhouette_rays.py all       # each part in a process of its own

Prints one JSON line per part."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _masks(n, H=224, W=224, seed=0):
    import numpy as np
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W), np.float32)
    for i in range(n):
        for _ in range(rng.randint(1, 4)):
            cy, cx, r = rng.uniform(40, 184), rng.uniform(40, 184), rng.uniform(15, 80)
            out[i] = np.maximum(out[i], ((yy - cy) ** 2 + (xx - cx) ** 2 < r * r).astype(np.float32))
    return out


def device(iters=200, warmup=20):
    import torch
    from shapeclipper_amd import ops
    dev = torch.device("cuda:0")
    masks = torch.from_numpy(_masks(192)).to(dev)
    seeds = torch.arange(192, dtype=torch.int64, device=dev) * 7919
    run = lambda: ops.silhouette_rays(ops.silhouette_distance(masks), 512, 5.0, seeds)
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    times = {}
    for name, fn in (("distance", lambda: ops.silhouette_distance(masks)), ("draw", None), ("both", run)):
        if name == "draw":
            dist = ops.silhouette_distance(masks)
            fn = lambda: ops.silhouette_rays(dist, 512, 5.0, seeds)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        e.synchronize()
        times[name] = s.elapsed_time(e) / iters
    return dict(part="device", masks=192, H=224, W=224, n_rays=512, ms_distance=round(times["distance"], 4),
                ms_draw=round(times["draw"], 4), ms_per_step=round(times["both"], 4))


def host(n=64):
    import numpy as np
    import torch
    from shapeclipper_amd.utils import util
    from shapeclipper_amd.utils.util import EasyDict as edict
    opt = edict(H=224, W=224, render=edict(rand_sample=512))
    masks = torch.from_numpy(_masks(n))
    np.random.seed(0)
    util.compute_sampling_prob(opt, masks[0], 5)
    t = time.perf_counter()
    for i in range(n):
        util.compute_sampling_prob(opt, masks[i], 5)
    ms = (time.perf_counter() - t) * 1e3 / n
    return dict(part="host", H=224, W=224, n_rays=512, ms_per_mask=round(ms, 3), ms_per_sample_K5=round(6 * ms, 2))


def loader(n_batches=16, batch_size=16, workers=16):
    import torch
    from shapeclipper_amd.data import pix3d_mini
    from shapeclipper_amd.utils import options
    import data.pix3d as pix3d
    torch.set_num_threads(1)
    out = dict(part="loader", workers=workers, batch_size=batch_size, image_size=224, k_nearest=5)
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "Pix3D")
        pix3d_mini.write_tree(root, n_per_cat=128, size=(224, 224), k_nearest=5, cat_key="chair,sofa", n_points=10000)
        for mode in ("on", "off", "on", "off"):                 # alternated; the better of the two runs of each mode is kept
            opt = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=perf_loader",
                                                       "--output_root=%s/out" % tmp, "--data.pix3d.cat=chair,sofa",
                                                       "--data.pix3d.root=%s" % root, "--data.num_workers=%d" % workers,
                                                       "--batch_size=%d" % batch_size, "--cpu"]
                                                      + ([] if mode == "on" else ["--hip.device_rays!"])), verbose=False)
            opt.world_size = 1
            ds = pix3d.Dataset(opt, split="train")
            it = iter(ds.setup_loader(opt, shuffle=True))
            next(it)                                        # worker start-up
            t = time.perf_counter()
            for _ in range(n_batches - 1):
                next(it)
            rate = round((n_batches - 1) * batch_size / (time.perf_counter() - t), 1)
            out["samples_per_s_device_rays_" + mode] = max(rate, out.get("samples_per_s_device_rays_" + mode, 0))
            del it
    return out


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what == "loader":
        os.environ["HIP_VISIBLE_DEVICES"] = os.environ["CUDA_VISIBLE_DEVICES"] = ""       # no device in the forking process
    if what == "all":
        for part in ("device", "host", "loader"):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), part])
        return
    print(json.dumps(dict(device=device, host=host, loader=loader)[what]()), flush=True)


if __name__ == "__main__":
    main()
