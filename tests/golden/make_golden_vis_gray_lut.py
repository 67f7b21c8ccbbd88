#!/usr/bin/env python
"""Generate tests/golden/vis_gray_lut.npz: how the reference turns a one-channel map into GIF bytes (build container only: needs
matplotlib, which the product does not import).

The reference's dump_gifs (utils/util_vis.py:68-75) clamps the map to [0, 1] (preprocess_vis_image), colours it with
plt.get_cmap("gray") (get_heatmap, :77-80: float64 RGBA -> RGB -> torch .float()) and writes (img * 255).astype(np.uint8).  Stored:
  lut_rgb    float64 [256, 3]  the colormap's table (integer input looks the table up directly)
  bad_rgb    float64 [3]       the colour of NaN
  x          float32 [N]       probe values: every k / 256 and its two fp32 neighbours, a 1 / 4096 grid, out-of-range values, -0, +-inf, NaN
  bytes      uint8   [N, 3]    the reference's bytes for each probe
  matplotlib the version that produced them.  Fixtures are data.

    python tests/golden/make_golden_vis_gray_lut.py
"""
import os

import matplotlib
import numpy as np
import torch

matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("GOLDEN_OUT", HERE)


def probes():
    k = np.arange(257, dtype=np.float32) / np.float32(256)
    edges = np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2))])
    grid = np.arange(4097, dtype=np.float32) / np.float32(4096)
    special = np.array([-0.0, -1e-7, -0.5, -3.0, 1.0000001, 1.5, 2.0, 1e30, -1e30, np.inf, -np.inf, np.nan, 0.5], np.float32)
    return np.concatenate([edges, grid, special]).astype(np.float32)


def reference_bytes(x):
    gray = torch.from_numpy(x).view(1, 1, 1, -1)                            # a [B, 1, H, W] map of one row, as dump_gifs sees a view
    gray = ((gray - 0) / (1 - 0)).clamp(min=0, max=1)                       # preprocess_vis_image, from_range (0, 1)
    color = plt.get_cmap("gray")(gray[:, 0].numpy())                        # get_heatmap
    color = torch.from_numpy(color[..., :3]).permute(0, 3, 1, 2).contiguous().float()
    img = color[0].permute(1, 2, 0).contiguous().numpy()                    # [1, W, 3]
    return (img * 255).astype(np.uint8)[0]


def main():
    cmap = plt.get_cmap("gray")
    x = probes()
    np.savez_compressed(os.path.join(OUT, "vis_gray_lut.npz"), lut_rgb=cmap(np.arange(256))[:, :3], bad_rgb=np.asarray(cmap(np.nan))[:3],
                        x=x, bytes=reference_bytes(x), matplotlib=np.array(matplotlib.__version__))
    print("wrote", os.path.join(OUT, "vis_gray_lut.npz"))


if __name__ == "__main__":
    main()
