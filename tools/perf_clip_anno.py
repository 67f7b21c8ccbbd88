#!/usr/bin/env python
"""Throughput of the Pix3D CLIP annotator (CLIP_anno.py's per-split loop: loader workers -> preprocessing -> tower) with both
preprocessing paths, on a generated tree of realistic source images (shapeclipper_amd/data/pix3d_mini.py; default 640 x 480).

    python tools/perf_clip_anno.py [--n 320] [--size 640x480] [--workers 16] [--batch 32] [--model ViT-B/32] [--out result.json]

Per path: one untimed pass over the split (worker start-up, tables, kernels), then timed passes; img/s = images / wall time of a pass,
ending with a device synchronisation.  Also times the tower alone on device-resident inputs and ops.clip_preprocess alone."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=320)
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--model", default="ViT-B/32")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.split("x"))
    import CLIP_anno
    import data.pix3d as pix3d
    from shapeclipper_amd.data import pix3d_mini
    from shapeclipper_amd.data.clip_preprocess import ClipPreprocess
    from shapeclipper_amd.utils import options

    tmp = tempfile.mkdtemp(prefix="perf_clip_anno_")
    root = os.path.join(tmp, "Pix3D")
    t0 = time.time()
    pix3d_mini.write_tree(root, n_per_cat=args.n // 2, size=(W, H), k_nearest=5, cat_key="chair,sofa", n_points=16, splits=("train",))
    print("tree: %d images of %dx%d in %.1f s" % (args.n, W, H, time.time() - t0), flush=True)
    result = dict(images=args.n, source=[W, H], workers=args.workers, batch=args.batch, model=args.model)
    for mode in ("device", "cpu"):
        argv = ["--yaml=%s/options/clip/pix3d.yaml" % ROOT, "--name=perf", "--output_root=%s/out" % tmp, "--data.pix3d.root=%s" % root,
                "--data.pix3d.cat=chair,sofa", "--batch_size=%d" % args.batch, "--data.num_workers=%d" % args.workers,
                "--clip_model=%s" % args.model] + ([] if mode == "device" else ["--hip.device_clip_preprocess!"])
        opt = options.set(options.parse_arguments(argv), verbose=False)
        ann = CLIP_anno.NN_annotator(opt)
        pre = ClipPreprocess(ann.n_px, opt.data.bgcolor)
        ds = pix3d.Dataset(opt, split="train", transform=pre)
        loader = torch.utils.data.DataLoader(ds, batch_size=opt.batch_size, num_workers=opt.data.num_workers, shuffle=False,
                                             drop_last=False, pin_memory=True, persistent_workers=True)

        def one_pass():
            if mode == "device":
                batches = (pre.device(b["rgba_input"].to(opt.device, non_blocking=True)) for b in loader)
            else:
                batches = (b["rgb_input"].to(opt.device, non_blocking=True) for b in loader)
            t = time.perf_counter()
            feats = ann.embed_batches(opt, batches)
            torch.cuda.synchronize()
            return time.perf_counter() - t, feats

        one_pass()
        times = [one_pass()[0] for _ in range(args.passes)]
        result["%s_img_per_s" % mode] = [round(args.n / t, 1) for t in times]
        print(mode, result["%s_img_per_s" % mode], flush=True)
        if mode == "device":
            rgba = torch.stack([ds[i]["rgba_input"] for i in range(args.batch)]).cuda()
            x = pre.device(rgba)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for what, fn in (("preprocess", lambda: pre.device(rgba)), ("tower", lambda: ann.tower.encode_image(x))):
                for _ in range(3):
                    fn()
                s.record()
                for _ in range(20):
                    fn()
                e.record()
                torch.cuda.synchronize()
                result["%s_ms_per_batch" % what] = round(s.elapsed_time(e) / 20, 4)
            print(result, flush=True)
        del loader
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
