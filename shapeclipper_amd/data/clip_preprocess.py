"""The CLIP tower's input from a Pix3D loader image (CLIP-annotation mode of data/pix3d.py), as the reference builds it.

Reference: data/pix3d.py:278-289 with a transform -- to_tensor, mask = a > 0.5, rgb = rgb * mask + bgcolor * (1 - mask),
to_pil_image (mul(255).byte(): truncation) -- then openai/CLIP's _transform(n_px): Resize(n_px, BICUBIC) (short side to n_px, long
side int(n_px * long / short), Pillow's resize), CenterCrop(n_px) (offsets int(round((size - n_px) / 2.0)), half to even), ToTensor and
Normalize(MEAN, STD) (sub, then div, in fp32).

Two ways to compute it, equal bit for bit:
  * `ClipPreprocess(n_px, bgcolor)(image)`: the CPU chain on one PIL RGBA image (PIL and torch ops), run in the loader's workers with
    `--hip.device_clip_preprocess!`;
  * `ClipPreprocess.device(rgba)` -> ops.clip_preprocess: a batch of uint8 RGBA images on the device (csrc/clip_preprocess.hip).  The
    kernel only does integer multiply-adds; its tables come from `bicubic_coeffs`, Pillow's recipe (libImaging/Resample.c,
    precompute_coeffs + normalize_coeffs_8bpc) restated in float64 in the same order of operations, built once per (H, W, n_px)."""
import functools

import numpy as np
import PIL.Image
import torch

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
PRECISION_BITS = 22                     # Pillow's 8-bit resampler: 32 - 8 - 2


def resize_size(h, w, n_px):
    """(new_h, new_w) of torchvision's Resize(n_px) on an h x w image: the short side becomes n_px, the long one int(n_px * long / short)."""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = n_px, int(n_px * long / short)
    return (new_long, new_short) if w <= h else (new_short, new_long)


def crop_offsets(h, w, n_px):
    """(top, left) of torchvision's CenterCrop(n_px) on an h x w image (h, w >= n_px): Python's round, half to even."""
    return int(round((h - n_px) / 2.0)), int(round((w - n_px) / 2.0))


def _bicubic(x):
    """Pillow's bicubic_filter (a = -0.5) on a float64 array, in its order of operations."""
    a = -0.5
    x = np.abs(x)
    inner = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    outer = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, inner, np.where(x < 2.0, outer, 0.0))


def bicubic_coeffs(in_size, out_size):
    """Pillow's coefficients for resizing one axis from in_size to out_size with BICUBIC: bounds [out_size, 2] int32 (first input
    pixel, tap count) and kk [out_size, ksize] int32 fixed point (2^22 = 1), zero past the tap count."""
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = _bicubic((np.arange(xmax, dtype=np.float64) + xmin - center + 0.5) * ss)
        ww = 0.0
        for v in w:                     # sequential sum, as the C loop
            ww += v
        if ww != 0.0:
            w = w / ww
        kk[xx, :xmax] = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)).astype(np.int32)
        bounds[xx] = xmin, xmax
    return bounds, kk


def resample_axis(img, bounds, kk, axis):
    """One pass of Pillow's 8-bit resampler on a uint8 array along `axis` (0: rows / vertical, 1: columns / horizontal)."""
    x = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((len(bounds),) + x.shape[1:], np.int64)
    for i, (start, count) in enumerate(bounds):
        k = kk[i, :count].astype(np.int64).reshape((count,) + (1,) * (x.ndim - 1))
        out[i] = (1 << (PRECISION_BITS - 1)) + (x[start:start + count] * k).sum(0)
    out = np.clip(out >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_numpy(img, size):
    """PIL.Image.resize(size=(W, H), BICUBIC) of an 8-bit image without alpha (uint8 [H, W] or [H, W, C]): horizontal pass first, a
    pass skipped when its axis keeps its size."""
    W, H = size
    out = img
    if W != img.shape[1]:
        out = resample_axis(out, *bicubic_coeffs(img.shape[1], W), axis=1)
    if H != img.shape[0]:
        out = resample_axis(out, *bicubic_coeffs(img.shape[0], H), axis=0)
    return out


def _axis_table(size, new_size, offset, n_px):
    """The kernel's table of one axis: resized pixels offset .. offset + n_px - 1 (the centre crop); an axis that keeps its size gets
    the identity (one tap of weight 2^22), which reproduces the skipped pass bit for bit."""
    if new_size == size:
        bounds = np.stack([np.arange(n_px, dtype=np.int32) + offset, np.ones(n_px, np.int32)], 1)
        kk = np.full((n_px, 1), 1 << PRECISION_BITS, np.int32)
    else:
        bounds, kk = bicubic_coeffs(size, new_size)
        bounds, kk = bounds[offset:offset + n_px], kk[offset:offset + n_px]
    return np.ascontiguousarray(bounds), np.ascontiguousarray(kk)


@functools.lru_cache(maxsize=64)
def kernel_tables(H, W, n_px):
    """(h_bounds, h_coef, v_bounds, v_coef) int32 numpy arrays of sc_clip_preprocess for H x W images."""
    new_h, new_w = resize_size(H, W, n_px)
    top, left = crop_offsets(new_h, new_w, n_px)
    return _axis_table(W, new_w, left, n_px) + _axis_table(H, new_h, top, n_px)


def background_byte(bgcolor):
    """The quantised background: to_pil_image's mul(255).byte() of the fp32 composite, trunc(fp32(bgcolor) * 255); -1 for None."""
    if bgcolor is None:
        return -1
    return int(np.trunc(np.float32(bgcolor) * np.float32(255)))


class ClipPreprocess:
    """transform of data/pix3d.py's CLIP-annotation mode: steps 2-4 of the reference on the loader's resized RGBA image."""

    def __init__(self, n_px=224, bgcolor=1):
        if bgcolor is not None and not 0.0 <= float(bgcolor) <= 1.0:
            raise ValueError("ClipPreprocess: bgcolor must be None or in [0, 1], got %r" % (bgcolor,))
        self.n_px = int(n_px)
        self.bgcolor = None if bgcolor is None else float(bgcolor)
        self._tables = {}

    def quantize(self, rgba):
        """uint8 [H, W, 4] -> uint8 [H, W, 3]: to_tensor, threshold, composite and to_pil_image in fp32 torch ops, as the reference."""
        t = torch.from_numpy(np.array(rgba, dtype=np.uint8)).permute(2, 0, 1).float().div(255)
        rgb, mask = t[:3], t[3:]
        mask = (mask > 0.5).float()
        if self.bgcolor is not None:
            rgb = rgb * mask + self.bgcolor * (1 - mask)
        return rgb.mul(255).byte().permute(1, 2, 0).contiguous().numpy()

    def __call__(self, image):
        """PIL RGBA image -> fp32 [3, n_px, n_px] on the CPU."""
        rgb = PIL.Image.fromarray(self.quantize(np.array(image.convert("RGBA"), dtype=np.uint8)), "RGB")
        new_h, new_w = resize_size(rgb.height, rgb.width, self.n_px)
        if (new_h, new_w) != (rgb.height, rgb.width):
            rgb = rgb.resize((new_w, new_h), PIL.Image.BICUBIC)
        top, left = crop_offsets(new_h, new_w, self.n_px)
        rgb = rgb.crop((left, top, left + self.n_px, top + self.n_px))
        x = torch.from_numpy(np.array(rgb, dtype=np.uint8)).permute(2, 0, 1).contiguous().float().div(255)
        mean = torch.tensor(MEAN, dtype=torch.float32)[:, None, None]
        std = torch.tensor(STD, dtype=torch.float32)[:, None, None]
        return x.sub(mean).div(std)

    def tables(self, H, W, device):
        """The kernel tables for H x W images as int32 tensors on `device`, kept per (H, W, device)."""
        key = (H, W, str(device))
        if key not in self._tables:
            self._tables[key] = tuple(torch.from_numpy(a).to(device) for a in kernel_tables(H, W, self.n_px))
        return self._tables[key]

    def device(self, rgba):
        """uint8 [B, H, W, 4] on the device -> fp32 [B, 3, n_px, n_px] (ops.clip_preprocess), equal to __call__ image by image."""
        from .. import ops
        return ops.clip_preprocess(rgba, self.n_px, self.bgcolor, tables=self.tables(rgba.shape[1], rgba.shape[2], rgba.device))
