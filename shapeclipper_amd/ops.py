"""Thin Python wrappers over the C ABI (allocation + pointer plumbing only; no arithmetic here)."""
from __future__ import annotations

import collections
import ctypes
import math
import weakref

import numpy as np
import torch

from . import _lib
from .mesh_pack import PackedMesh, check_counts, check_mesh_tensors, check_packed, check_starts, device_tensor
from .packing import n_tiles

_SCRATCH = {}       # (tag, device index, raw stream) -> fp32 buffer; every cached device scratch of this module lives here


def _scratch(tag, dev, n_floats):
    """The fp32 scratch buffer `tag` of at least n_floats for torch's current stream on `dev`: one per (tag, device, stream) -- calls on
    a stream are ordered, so they can share it -- grown on demand, never shrunk.  Uses that were separate buffers carry separate tags;
    the tags of buffers whose size follows the convolution grid start with "conv" (set_reserved_cus drops those).  The stream is read
    without touching the device ptr() remembers, so the device guard of the launch itself judges the call's tensors."""
    if dev.type != "cuda":
        raise RuntimeError(_lib.NO_CPU)
    key = (tag, dev.index, torch._C._cuda_getCurrentRawStream(dev.index))
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() < n_floats:
        buf = _SCRATCH[key] = torch.empty(n_floats, device=dev, dtype=torch.float32)
    return buf


SDF_SCRATCH_FLOATS = 256 * 8 * 5 * 1024     # sc_sdf_forward's parked pre-activations: [256 workgroups x 8 waves][5][1024] floats (42 MB)
_stream_imgs = {}                           # id(w_pack) -> (weak reference to w_pack, its _version, raw stream, image)


def _sdf_stream_image(w_pack):
    """The pre-split fragment image of sc_sdf_forward_stream for this packed weight tensor.  The four SDF calls of a training step (two renders,
    two eikonal batches) share ONE w_pack tensor (SDFNetwork.packed): the image is built once for it.  A hit needs the SAME tensor object at
    the same version on the same stream.  The entry holds the pack weakly and goes when the pack does (its address is a key only while
    it lives), so neither the pack nor the graph behind it is kept alive, and packs that alternate on a stream each keep their image.
    A pack must NOT be rewritten in place through raw pointers (the C ABI): that does not bump _version and would leave a stale image."""
    _lib.ptr(w_pack)                    # (a CPU tensor is refused here with the product's own message: there is no CPU fallback)
    key, st = id(w_pack), _lib.raw_stream()
    hit = _stream_imgs.get(key)
    if hit is not None and hit[0]() is w_pack and hit[1:3] == (w_pack._version, st):
        return hit[3]
    lib = _lib.load()
    img = torch.empty(lib.sc_sdf_stream_pack_bytes(), device=w_pack.device, dtype=torch.uint8)
    _lib.check(lib.sc_sdf_stream_pack(_lib.ptr(w_pack), _lib.ptr(img), _lib.stream()), "sc_sdf_stream_pack")
    _stream_imgs[key] = (weakref.ref(w_pack, lambda _, key=key: _stream_imgs.pop(key, None)), w_pack._version, st, img)
    return img


RGB_BWD_SPLIT = True      # reverse chain of the RGB network (fused form that reads the parked activations) from pre-split transposed fragments
RGB_FWD_SPLIT = True      # RGB network of the forward pass from pre-split bf16x3 fragments (csrc/rgb_fwd.hip, mlp_presplit.hpp); False: fp32 MFMA
SDF_FWD_STREAM = True     # sdf_forward with d sdf/dx from streamed pre-split fragments (csrc/sdf_fwd_stream.hip); False: sdf_fwd.hip (fp32 MFMA)
SDF_VALUE_SPLIT = True    # value-only SDF calls (no gradient, no feature, no stash) take csrc/sdf_value_split.hip; False: sdf_fwd.hip (fp32 MFMA)
FUSED_RGB_WGRAD = True    # `--hip.fused_rgb_wgrad!`: Gy_l / r_l through HBM and three sc_wgrad launches (the round-4 path)
RGB_STASH = True          # `--hip.rgb_stash!`: the backward recomputes the RGB forward chain instead of loading r0..r2 parked by the forward


def sdf_forward_entry(want_grad: bool, want_feat: bool, stash: bool) -> str:
    """The entry point sdf_forward calls for these outputs under the switches above.  Pure host logic."""
    if SDF_VALUE_SPLIT and not (want_grad or want_feat or stash):
        return "sc_sdf_value_forward_split"
    if SDF_FWD_STREAM and want_grad and (not stash or want_feat):
        return "sc_sdf_forward_stream"
    return "sc_sdf_forward"


def rgb_reverse_form(n_images: int, parked: bool) -> str:
    """The entry-point stem of rgb_composite_backward (_entry adds _ns for S != 64) for a batch of n_images, `parked`: the forward kept
    r0..r2.  The fused kernels take at most 256 images (csrc/rgb_bwd.hip).  Pure host logic."""
    if not (FUSED_RGB_WGRAD and n_images <= 256):
        return "sc_rgb_composite_backward_v3"
    if not parked:
        return "sc_rgb_composite_backward_fused"
    return "sc_rgb_composite_backward_fused_" + ("split" if RGB_BWD_SPLIT else "stash")


def rgb_forward_parks(n_images: int) -> bool:
    """Whether a forward that needs gradients parks r0..r2 (805 MB per bs32 render): only when the reverse pass will load them."""
    return bool(RGB_STASH) and rgb_reverse_form(n_images, True) != "sc_rgb_composite_backward_v3"


def sdf_forward(points: torch.Tensor, w_pack: torch.Tensor, cbias: torch.Tensor, n_per_image: int,
                symmetric: bool = True, want_grad: bool = True, want_feat: bool = True,
                stash: bool = False):
    """points [N,3] -> (sdf [N], grad [N,3] | None, feat TBL64 | None[, stash_a, stash_p])."""
    lib = _lib.load()
    n = points.shape[0]
    dev = points.device
    nt = n_tiles(n)
    sdf = torch.empty(n, device=dev, dtype=torch.float32)
    name = sdf_forward_entry(want_grad, want_feat, stash)
    if name == "sc_sdf_value_forward_split":
        # the value alone (compute_level_grid): the chain in the exact bf16x3 split arithmetic with pre-split weights, 1.6x the fp32-MFMA
        # chain (csrc/sdf_value_split.hip, profiles/r06_value_chain_split_ab.txt)
        _lib.check(lib.sc_sdf_value_forward_split(_lib.ptr(points), _lib.ptr(w_pack), _lib.ptr(cbias), n, n_per_image,
                                                  cbias.shape[0], 1 if symmetric else 0, _lib.ptr(sdf), _lib.stream()),
                   "sc_sdf_value_forward_split")
        return sdf, None, None
    grad = torch.empty(n, 3, device=dev, dtype=torch.float32) if want_grad else None
    feat = torch.empty(nt * 1024, device=dev, dtype=torch.float32) if want_feat else None
    sa = torch.empty(5 * nt * 1024, device=dev, dtype=torch.float32) if stash else None
    sp = torch.empty(4 * nt * 1024, device=dev, dtype=torch.float32) if (stash and want_grad) else None
    # gradient kernel without a training stash: per-wave scratch for the parked pre-activations (L2-resident)
    scratch = _scratch("sdf", dev, SDF_SCRATCH_FLOATS) if (want_grad and not stash) else None
    # sc_sdf_forward_stream: value + feature + d sdf/dx from pre-split bf16x3 fragments streamed through LDS (csrc/sdf_fwd_stream.hip),
    # the same arguments with the fragment image after the points
    img = (_lib.ptr(_sdf_stream_image(w_pack)),) if name == "sc_sdf_forward_stream" else ()
    code = getattr(lib, name)(_lib.ptr(points), *img, _lib.ptr(w_pack), _lib.ptr(cbias), n, n_per_image, cbias.shape[0],
                              1 if symmetric else 0, _lib.ptr(sdf), _lib.ptr(grad), _lib.ptr(feat), _lib.ptr(sa), _lib.ptr(sp),
                              _lib.ptr(scratch), _lib.stream())
    _lib.check(code, name)
    if stash:
        return sdf, grad, feat, sa, sp
    return sdf, grad, feat


def rgb_composite_forward(points, z_vals, depth_fac, sdf, grad, feat, v_pack, dbias, beta_param,
                          rays_per_image: int, symmetric: bool, beta_min: float, bgcolor: float,
                          normal_pow: float, keep_samples: bool = False, keep_rgb_flat: bool = False, keep_rr: bool = False):
    """Per-ray outputs of the renderer from the per-point SDF results.

    points [n_rays*S,3], z_vals [n_rays,S], depth_fac [n_rays], sdf [P], grad [P,3], feat TBL64 (P = n_rays*S,
    S = samples per ray, sample_count_supported(S)).
    Returns dict(rgb [n_rays,3], mask, mask_hard, depth [n_rays], normal [n_rays,3]
    [, weights, alpha [n_rays,S], rgb_flat [P,3]])."""
    lib = _lib.load()
    n_rays, S = z_vals.shape
    if not sample_count_supported(S):
        raise ValueError("shapeclipper_amd: the compositing kernels take S %% 32 == 0, 32 <= S <= 256 samples per ray, not %d" % S)
    dev = points.device
    f32 = dict(device=dev, dtype=torch.float32)
    out = dict(rgb=torch.empty(n_rays, 3, **f32), mask=torch.empty(n_rays, **f32),
               mask_hard=torch.empty(n_rays, **f32), depth=torch.empty(n_rays, **f32),
               normal=torch.empty(n_rays, 3, **f32))
    if keep_samples:
        out.update(weights=torch.empty(n_rays, S, **f32), alpha=torch.empty(n_rays, S, **f32))
    if keep_samples or keep_rgb_flat:
        out.update(rgb_flat=torch.empty(n_rays * S, 3, **f32))
    if keep_rr:      # the hidden activations r0, r1, r2 (3 x TBL64) for rgb_composite_backward(rr=...): 805 MB per bs32 render at S = 64
        out.update(rr=torch.empty(3 * n_rays * (S // 16) * 1024, **f32))
    # round 6: the RGB network from pre-split bf16x3 weight fragments (csrc/rgb_fwd.hip, `--hip.rgb_split!` keeps the fp32-MFMA chain)
    name = "sc_rgb_composite_forward_split" if RGB_FWD_SPLIT else "sc_rgb_composite_forward_stash"
    fwd, ns = _entry(lib, name, S)
    code = fwd(
        _lib.ptr(points), _lib.ptr(z_vals), _lib.ptr(depth_fac), _lib.ptr(sdf), _lib.ptr(grad), _lib.ptr(feat),
        _lib.ptr(v_pack), _lib.ptr(dbias), _lib.ptr(beta_param), n_rays, *ns, rays_per_image,
        dbias.shape[0], 1 if symmetric else 0, beta_min, bgcolor,
        normal_pow, _lib.ptr(out["rgb"]), _lib.ptr(out["mask"]), _lib.ptr(out["mask_hard"]),
        _lib.ptr(out["depth"]), _lib.ptr(out["normal"]), _lib.ptr(out.get("weights")), _lib.ptr(out.get("alpha")),
        _lib.ptr(out.get("rgb_flat")), _lib.ptr(out.get("rr")), _lib.stream())
    _lib.check(code, name)
    return out


def rgb_points_forward(points, grad, feat, v_pack, dbias, n_per_image: int, symmetric: bool, want_rgb: bool = True,
                       want_normal: bool = True):
    """RGBNetwork.forward and the unit SDF normal at arbitrary points (mesh vertices), from the sdf_forward outputs of those points.

    points [N,3], grad [N,3] (read for the normal), feat TBL64 (read for the colour), v_pack / dbias [n_images,3,64] (RGBNetwork.packed);
    point i belongs to image (16 * (i // 16)) // n_per_image, n_per_image a multiple of 16 (the layout of sdf_forward(n_per_image=...)).
    -> (rgb [N,3] sigmoid colours | None, normal [N,3] = grad / max(|grad|, 1e-12) | None).  The colours are those of
    rgb_composite_forward's rgb_flat bit for bit (the same pre-split bf16x3 chain, csrc/rgb_points.hip).  No autograd: inference only."""
    if n_per_image <= 0 or n_per_image % 16:
        raise ValueError("shapeclipper_amd: rgb_points_forward needs n_per_image to be a positive multiple of 16, not %d" % n_per_image)
    n = points.shape[0]
    if points.shape != (n, 3) or (want_normal and grad.numel() < 3 * n) or (want_rgb and feat.numel() < n_tiles(n) * 1024):
        raise ValueError("shapeclipper_amd: rgb_points_forward takes points [N,3], grad [N,3] and feat of ceil(N / 16) TBL64 tiles")
    lib = _lib.load()
    f32 = dict(device=points.device, dtype=torch.float32)
    rgb = torch.empty(n, 3, **f32) if want_rgb else None
    normal = torch.empty(n, 3, **f32) if want_normal else None
    code = lib.sc_rgb_points_forward_split(
        _lib.ptr(points), _lib.ptr(grad if want_normal else None), _lib.ptr(feat if want_rgb else None),
        _lib.ptr(v_pack if want_rgb else None), _lib.ptr(dbias if want_rgb else None), n, n_per_image,
        dbias.shape[0] if want_rgb else 1, 1 if symmetric else 0, _lib.ptr(rgb), _lib.ptr(normal), _lib.stream())
    _lib.check(code, "sc_rgb_points_forward_split")
    return rgb, normal


def _entry(lib, name, S):
    """The entry point `name` for S samples per ray and the sample-count argument it takes after n_rays: S = 64 calls the symbol
    without the count (the kernels of the default, and the names bench.py and profiles know), any other S its _ns twin."""
    return (getattr(lib, name), ()) if S == 64 else (getattr(lib, name + "_ns"), (S,))


def sample_count_supported(n_samples: int) -> bool:
    """Samples per ray the render kernels take (SC_N_SAMPLES_SUPPORTED): a multiple of 32 in [32, 256] -- 1 to 4 chunks of 64 samples
    per ray, the last one possibly half a wave.  Pure host logic."""
    return isinstance(n_samples, int) and 32 <= n_samples <= 256 and n_samples % 32 == 0


# operand transform codes of sc_wgrad (csrc/wgrad.hip)
OP_NONE, OP_PLAIN, OP_SP, OP_Q, OP_Q4, OP_PE, OP_EPS = range(7)
WGRAD_PARTS = 512
RGB_BWD_BETA_PARTS = 2048      # SC_RGB_BWD_BETA_PARTS (include/shapeclipper_hip.h)


def _partial_reduce(lib, partial, nparts, stride, n, out):
    """out[:n] = sum over the parts in a fixed order (csrc/wgrad.hip partial_reduce_kernel: no atomics)."""
    _lib.check(lib.sc_partial_reduce(_lib.ptr(partial), nparts, stride, n, _lib.ptr(out), _lib.stream()),
               "sc_partial_reduce")
    return out


def _wgrad(lib, terms, points, g_grad, w5row, n_points, symmetric, nb0, nb1, partial, stride, out_offset, out_ld,
           rowsum=None, n_per_image=0, n_images=0):
    """terms: list of 1 or 2 tuples (a0, a1, aop, b0, bop0, b1, bop1).  rowsum [n_images,64] (any content): receives the per-image
    sum of term 0's A operand, produced on the way -- every wave of the grid writes its own partial image and the partials are
    added in index order (fixed summation order)."""
    t = list(terms) + [(None, None, OP_NONE, None, OP_NONE, None, OP_NONE)] * (2 - len(terms))
    args = []
    for (a0, a1, aop, b0, bop0, b1, bop1) in t:
        args += [_lib.ptr(a0), _lib.ptr(a1), aop, _lib.ptr(b0), bop0, _lib.ptr(b1), bop1]
    rs_part = _scratch("rowsum", points.device, WGRAD_PARTS * 4 * n_images * 64) if rowsum is not None else None
    code = lib.sc_wgrad(len(terms), *args, _lib.ptr(points), _lib.ptr(g_grad), _lib.ptr(w5row),
                        n_points, 1 if symmetric else 0, nb0, nb1, _lib.ptr(partial),
                        WGRAD_PARTS, stride, out_offset, out_ld, _lib.ptr(rs_part),
                        n_per_image, n_images, _lib.stream())
    _lib.check(code, "sc_wgrad")
    if rowsum is not None:
        _partial_reduce(lib, rs_part, WGRAD_PARTS * 4, n_images * 64, n_images * 64, rowsum)


def tbl_sum_multi(xs, n_points, n_per_image, n_images, coef=None):
    """Per-image sums over the points of several TBL64 tensors in ONE launch
    -> [len(xs), n_images, K, 64] (K = 3 with coef [N,3], else 1)."""
    lib = _lib.load()
    K = 3 if coef is not None else 1
    n = len(xs)
    dev = xs[0].device
    PtrArr = ctypes.c_void_p * n
    xp = PtrArr(*[x.data_ptr() for x in xs])
    blocks = int(lib.sc_tbl_sum_blocks(n_points))
    fixed = n_per_image % 16 == 0 and blocks * n * n_images * K * 64 <= (1 << 26)     # partial images of at most 256 MB
    if fixed:       # fixed summation order: per-block partial images + an ordered sum
        out = torch.empty(n, n_images, K, 64, device=dev, dtype=torch.float32)
        part = _scratch("rowsum", dev, blocks * n * n_images * K * 64)
    else:           # images that are not whole tiles (per-point latents) or too many of them: float atomics
        out = torch.zeros(n, n_images, K, 64, device=dev, dtype=torch.float32)
        part = None
    op = PtrArr(*[out[i].data_ptr() for i in range(n)])
    code = lib.sc_tbl_sum(xp, n, _lib.ptr(coef), n_points, n_per_image, n_images, op, _lib.ptr(part),
                          _lib.stream())
    _lib.check(code, "sc_tbl_sum")
    return out


def tbl_sum(x, n_points, n_per_image, n_images, coef=None):
    return tbl_sum_multi([x], n_points, n_per_image, n_images, coef)[0]


def sdf_backward_fused(points, w_pack, n_per_image, n_images, symmetric, stash_a, stash_p, g_sdf, g_grad, g_feat,
                       want_points_grad=True):
    """csrc/sdf_bwdw.hip: input gradients and every weight / bias gradient of the SDF network in one launch."""
    from .packing import SDF_PACK_FLOATS
    lib = _lib.load()
    n = points.shape[0]
    dev = points.device
    f32 = dict(device=dev, dtype=torch.float32)
    if n == 0:          # nothing is launched for an empty point set: the gradients are zeros, not uninitialised partial images
        return (torch.zeros(0, 3, **f32) if want_points_grad else None), torch.zeros(SDF_PACK_FLOATS, **f32), torch.zeros(n_images, 5, 64, **f32)
    for t in (g_sdf, g_grad, g_feat):
        if t is not None and not (t.is_contiguous() and t.dtype == torch.float32):
            raise RuntimeError("shapeclipper_amd: sc_sdf_backward_fused needs contiguous fp32 upstream gradients")
    parts = int(lib.sc_sdf_backward_fused_parts(n))
    stride = int(lib.sc_sdf_backward_fused_partial_floats(n_images))
    dense = stride > SDF_PACK_FLOATS                  # per-image bias gradients ride in the partial images (fixed summation order)
    park = _scratch("park", dev, 256 * 4 * 4 * 1024)      # the parked second-order terms (L2-resident)
    partial = torch.empty(parts * stride, **f32)
    g_c = None if dense else torch.zeros(n_images, 5, 64, **f32)
    g_points = torch.empty(n, 3, **f32) if want_points_grad else None
    code = lib.sc_sdf_backward_fused(_lib.ptr(points), _lib.ptr(w_pack), n, n_per_image, n_images,
                                     1 if symmetric else 0, _lib.ptr(stash_a), _lib.ptr(stash_p), _lib.ptr(g_sdf),
                                     _lib.ptr(g_grad), _lib.ptr(g_feat), _lib.ptr(g_points), _lib.ptr(park),
                                     _lib.ptr(partial), _lib.ptr(g_c), _lib.stream())
    _lib.check(code, "sc_sdf_backward_fused")
    g_all = _partial_reduce(lib, partial, parts, stride, stride, torch.empty(stride, **f32))
    if dense:
        g_c = g_all[SDF_PACK_FLOATS:].view(n_images, 5, 64)
    return g_points, g_all[:SDF_PACK_FLOATS], g_c


def sdf_backward(points, w_pack, n_per_image, n_images, symmetric, stash_a, stash_p, g_sdf, g_grad, g_feat,
                 want_points_grad=True, fused=True):
    """Reverse pass of sdf_forward (incl. second-order terms) -> (g_points | None, g_w_pack, g_cbias).
    fused (hip.fused_backward): one workgroup-cooperative launch (csrc/sdf_bwdw.hip) when the d sdf/dx output is
    differentiated; otherwise sdf_bwd.hip + 8 wgrad.hip launches + tbl_sum through hand-off tensors in HBM."""
    from .packing import SDF_OFF, SDF_PACK_FLOATS
    if fused and g_grad is not None and stash_p is not None and n_per_image % 16 == 0:
        return sdf_backward_fused(points, w_pack, n_per_image, n_images, symmetric, stash_a, stash_p, g_sdf, g_grad,
                                  g_feat, want_points_grad)
    lib = _lib.load()
    n = points.shape[0]
    dev = points.device
    nt = n_tiles(n)
    T = nt * 1024
    f32 = dict(device=dev, dtype=torch.float32)
    ga = torch.empty(5 * T, **f32)
    gp = torch.empty(4 * T, **f32) if g_grad is not None else None
    r0 = torch.empty(T, **f32)
    g_points = torch.empty(n, 3, **f32) if want_points_grad else None
    code = lib.sc_sdf_backward(_lib.ptr(points), _lib.ptr(w_pack), n, 1 if symmetric else 0,
                               _lib.ptr(stash_a), _lib.ptr(stash_p), _lib.ptr(g_sdf), _lib.ptr(g_grad),
                               _lib.ptr(g_feat), _lib.ptr(g_points), _lib.ptr(ga), _lib.ptr(gp), _lib.ptr(r0),
                               _lib.stream())
    _lib.check(code, "sc_sdf_backward")

    A = lambda l: stash_a[l * T:(l + 1) * T]
    P = lambda l: stash_p[l * T:(l + 1) * T]
    GA = lambda l: ga[l * T:(l + 1) * T]
    GP = lambda l: gp[l * T:(l + 1) * T]
    gg = g_grad is not None
    stride = SDF_PACK_FLOATS
    partial = torch.empty(WGRAD_PARTS * stride, **f32)     # every workgroup of every launch writes its whole region
    w5row = w_pack[SDF_OFF["W5"]:SDF_OFF["W5"] + 64]
    common = (points, g_grad, w5row, n, symmetric)

    # per-image sums of Ga_l (the gradient of the per-image biases c_l) come out of the launch that streams Ga_l anyway
    fold = n_per_image % 16 == 0
    g_c5 = torch.empty(5, n_images, 64, **f32) if fold else None

    def launch(terms, nb0, nb1, off, ld, layer=None):
        rs = g_c5[layer] if (fold and layer is not None) else None
        _wgrad(lib, terms, *common, nb0, nb1, partial, stride, off, ld, rs, n_per_image, n_images)

    t = [(GA(0), None, OP_PLAIN, None, OP_PE, None, OP_NONE)]
    if gg:
        t.append((P(0), A(0), OP_Q, None, OP_EPS, None, OP_NONE))
    launch(t, 48, 0, SDF_OFF["W0"], 48, layer=0)
    for l, key in ((1, "W1"), (2, "W2")):      # [64][112] = [hidden 64 | PE 48]: two launches of <= 4 N tiles each
        t = [(GA(l), None, OP_PLAIN, A(l - 1), OP_SP, None, OP_NONE)]
        if gg:
            t.append((P(l), A(l), OP_Q, GP(l - 1), OP_PLAIN, None, OP_NONE))
        launch(t, 64, 0, SDF_OFF[key], 112, layer=l)
        t = [(GA(l), None, OP_PLAIN, None, OP_PE, None, OP_NONE)]
        if gg:
            t.append((P(l), A(l), OP_Q, None, OP_EPS, None, OP_NONE))
        launch(t, 48, 0, SDF_OFF[key] + 64, 112)
    t = [(GA(3), None, OP_PLAIN, A(2), OP_SP, None, OP_NONE)]
    if gg:
        t.append((P(3), A(3), OP_Q, GP(2), OP_PLAIN, None, OP_NONE))
    launch(t, 64, 0, SDF_OFF["W3"], 64, layer=3)
    t = [(GA(4), None, OP_PLAIN, A(3), OP_SP, None, OP_NONE)]
    if gg:
        t.append((None, A(4), OP_Q4, GP(3), OP_PLAIN, None, OP_NONE))
    launch(t, 64, 0, SDF_OFF["W4"], 64, layer=4)
    if g_feat is not None:
        launch([(g_feat, None, OP_PLAIN, A(4), OP_SP, None, OP_NONE)], 64, 0, SDF_OFF["W5"] + 64, 64)

    g_w = _partial_reduce(lib, partial, WGRAD_PARTS, stride, stride, torch.empty(stride, **f32))
    # W5 row 0 (sdf row):  sum_p (Gs * h4 + Gq4 * sp'(a4))   and the output bias
    tot = tbl_sum_multi([r0] + ([g_feat] if g_feat is not None else []), n, n, 1)
    g_w[SDF_OFF["W5"]:SDF_OFF["W5"] + 64] = tot[0].view(64)
    g_w[SDF_OFF["B5"]] = g_sdf.sum() if g_sdf is not None else 0.0
    if g_feat is not None:
        g_w[SDF_OFF["B5"] + 1:SDF_OFF["B5"] + 65] = tot[1].view(64)
    else:   # regions no launch wrote (the partial buffer is not zero-initialised)
        g_w[SDF_OFF["W5"] + 64:SDF_OFF["B5"]] = 0.0
        g_w[SDF_OFF["B5"] + 1:] = 0.0
    if fold:
        g_c = g_c5.permute(1, 0, 2).contiguous()
    else:
        g_c = tbl_sum_multi([GA(l) for l in range(5)], n, n_per_image, n_images).view(5, n_images, 64).permute(1, 0, 2).contiguous()
    return g_points, g_w, g_c


def rgb_composite_backward(points, z_vals, depth_fac, sdf, grad, feat, v_pack, dbias, beta_param, rgb_flat,
                           rays_per_image, symmetric, beta_min, bgcolor, normal_pow,
                           G_rgb, G_mask, G_depth, G_normal, rr=None):
    """Reverse pass of rgb_composite_forward.
    -> dict(points, z_vals, depth_fac, sdf, grad, feat, v_pack, dbias, beta) gradients."""
    from .packing import RGB_OFF, RGB_PACK_FLOATS
    lib = _lib.load()
    n_rays, S = z_vals.shape
    n_images = dbias.shape[0]
    P = n_rays * S
    T = n_rays * (S // 16) * 1024
    dev = points.device
    f32 = dict(device=dev, dtype=torch.float32)
    g = dict(sdf=torch.empty(P, **f32), grad=torch.empty(P, 3, **f32), feat=torch.empty(T, **f32),
             points=torch.empty(P, 3, **f32), z_vals=torch.empty(n_rays, S, **f32),
             depth_fac=torch.empty(n_rays, **f32), beta=torch.empty(RGB_BWD_BETA_PARTS, **f32))
    v3_part = torch.empty(RGB_BWD_BETA_PARTS * 196, **f32)     # per-wave partial sums of dV3 [3][64] | db3 [3] | 0
    # the arguments every reverse entry point starts with (S != 64: the sample count after n_rays, see _entry)
    head = (_lib.ptr(points), _lib.ptr(z_vals), _lib.ptr(depth_fac), _lib.ptr(sdf), _lib.ptr(grad), _lib.ptr(feat), _lib.ptr(v_pack),
            _lib.ptr(dbias), _lib.ptr(beta_param), _lib.ptr(rgb_flat), n_rays, *(() if S == 64 else (S,)), rays_per_image, n_images,
            1 if symmetric else 0, beta_min, bgcolor, normal_pow, _lib.ptr(G_rgb), _lib.ptr(G_mask), _lib.ptr(G_depth), _lib.ptr(G_normal),
            _lib.ptr(g["sdf"]), _lib.ptr(g["grad"]), _lib.ptr(g["feat"]), _lib.ptr(g["points"]), _lib.ptr(g["z_vals"]),
            _lib.ptr(g["depth_fac"]), _lib.ptr(g["beta"]))
    name = rgb_reverse_form(n_images, rr is not None)
    if name != "sc_rgb_composite_backward_v3":
        # round 5: the gradients of V0, V1, V2 and of the per-image biases are formed inside the kernel by four weight-gradient waves (the scheme
        # of sc_sdf_backward_fused): no Gy_l / r_l hand-off tensors (1.6 GB per bs32 render) and no sc_wgrad launches
        parts = int(lib.sc_rgb_composite_backward_fused_parts(n_rays))
        stride = int(lib.sc_rgb_composite_backward_fused_partial_floats(n_images))
        partial = torch.empty(parts * stride, **f32)
        # the forward parked r0..r2: no recomputation of the forward chain (_split: the reverse chain's transposed products from pre-split
        # bf16x3 fragments, `--hip.rgb_bwd_split!`: fp32 MFMA)
        tail = (_lib.ptr(rr),) if rr is not None else ()
        _lib.check(_entry(lib, name, S)[0](*head, _lib.ptr(partial), _lib.ptr(v3_part), *tail, _lib.stream()), name)
        g_all = _partial_reduce(lib, partial, parts, stride, stride, torch.empty(stride, **f32))
        g_v = torch.empty(RGB_PACK_FLOATS, **f32)
        g_v[:RGB_OFF["V3"]] = g_all[:RGB_OFF["V3"]]
        g["beta"] = _partial_reduce(lib, g["beta"], RGB_BWD_BETA_PARTS, 1, 1, torch.empty(1, **f32))
        assert RGB_OFF["B3"] == RGB_OFF["V3"] + 192 and RGB_PACK_FLOATS == RGB_OFF["B3"] + 4
        _partial_reduce(lib, v3_part, RGB_BWD_BETA_PARTS, 196, 196, g_v[RGB_OFF["V3"]:])
        g["v_pack"] = g_v
        g["dbias"] = g_all[RGB_OFF["V3"]:].view(n_images, 3, 64)
        return g
    gy = torch.empty(3 * T, **f32)
    rr = torch.empty(2 * T, **f32)         # r0, r1 (operands of dV1 / dV2); r2 and gy3 only feed the output layer's gradient, formed in the kernel:
    code = _entry(lib, name, S)[0](*head, _lib.ptr(gy), _lib.ptr(rr), None, _lib.ptr(v3_part), _lib.stream())
    _lib.check(code, name)

    GY = lambda l: gy[l * T:(l + 1) * T]
    RR = lambda l: rr[l * T:(l + 1) * T]
    stride = RGB_PACK_FLOATS
    partial = torch.empty(WGRAD_PARTS * stride, **f32)
    common = (points, None, None, P, symmetric)
    # per-image sums of Gy_l (gradient of the per-image biases d_l) are produced by the launch that streams Gy_l
    npi = rays_per_image * S
    g_d3 = torch.empty(3, n_images, 64, **f32)
    rs = lambda l: (g_d3[l], npi, n_images)
    # V0 = [PE 48 | sdf feature 64]: one launch (Gy0 is streamed once, 7 N tiles)
    _wgrad(lib, [(GY(0), None, OP_PLAIN, None, OP_PE, feat, OP_PLAIN)], *common, 48, 64, partial, stride, RGB_OFF["V0"], 112, *rs(0))
    _wgrad(lib, [(GY(1), None, OP_PLAIN, RR(0), OP_PLAIN, None, OP_NONE)], *common, 64, 0, partial, stride, RGB_OFF["V1"], 64, *rs(1))
    _wgrad(lib, [(GY(2), None, OP_PLAIN, RR(1), OP_PLAIN, None, OP_NONE)], *common, 64, 0, partial, stride, RGB_OFF["V2"], 64, *rs(2))
    g_v = _partial_reduce(lib, partial, WGRAD_PARTS, stride, stride, torch.empty(stride, **f32))
    g["beta"] = _partial_reduce(lib, g["beta"], RGB_BWD_BETA_PARTS, 1, 1, torch.empty(1, **f32))     # per-wave partials, index order
    # the 3-row output layer: [V3 (192) | b3 (3) | pad] is contiguous in the pack -- the per-wave partials of the kernel, summed in index order
    assert RGB_OFF["B3"] == RGB_OFF["V3"] + 192 and RGB_PACK_FLOATS == RGB_OFF["B3"] + 4
    _partial_reduce(lib, v3_part, RGB_BWD_BETA_PARTS, 196, 196, g_v[RGB_OFF["V3"]:])
    g["v_pack"] = g_v
    g["dbias"] = g_d3.permute(1, 0, 2).contiguous()
    return g


def loss_fused_forward(rgb, rgb_t, mask, mask_t, normal, normal_t, eik, normal_l1, mask_mse, keep_frac, want_target_grad=False):
    """-> (out [4] = (render, mask, normal, eikonal) losses, (g_rgb, g_mask, g_normal, g_eik|None, g_normal_t|None))."""
    lib = _lib.load()
    B, R = rgb.shape[0], rgb.shape[1]
    dev = rgb.device
    f32 = dict(device=dev, dtype=torch.float32)
    c = lambda t: t.detach().contiguous().float()
    rgb, rgb_t, normal, normal_t = c(rgb), c(rgb_t), c(normal), c(normal_t)
    mask, mask_t = c(mask).view(B, R), c(mask_t).view(B, R)
    E = 0
    if eik is not None:
        eik = c(eik).view(B, -1)
        E = eik.shape[1]
    out = torch.zeros(8, **f32)           # 4 losses | arrival counter of the fixed-order reduction (must start at zero) | pad
    g_rgb, g_mask, g_normal = torch.empty(B, R, 3, **f32), torch.empty(B, R, **f32), torch.empty(B, R, 3, **f32)
    g_eik = torch.empty(B, E, **f32) if eik is not None else None
    g_normal_t = torch.empty(B, R, 3, **f32) if want_target_grad else None
    ws = torch.empty(B * R + 4 * B, **f32)
    code = lib.sc_loss_fused_forward(_lib.ptr(rgb), _lib.ptr(rgb_t), _lib.ptr(mask), _lib.ptr(mask_t), _lib.ptr(normal),
                                     _lib.ptr(normal_t), _lib.ptr(eik), B, R, E,
                                     normal_l1, mask_mse, keep_frac,
                                     _lib.ptr(out), _lib.ptr(g_rgb), _lib.ptr(g_mask), _lib.ptr(g_normal),
                                     _lib.ptr(g_eik), _lib.ptr(g_normal_t), _lib.ptr(ws), _lib.stream())
    _lib.check(code, "sc_loss_fused_forward")
    return out[:4], (g_rgb, g_mask, g_normal, g_eik, g_normal_t)


def ray_sample_forward(cam_loc, ray_dirs, scale_dist, u, rays_per_image, cam_dist, n_samples=64):
    """-> z_vals [n_rays,S], points [n_rays*S,3]  (u [n_rays,S], or None: evaluation linspace; S = n_samples)."""
    lib = _lib.load()
    n_rays, S = ray_dirs.shape[0], int(n_samples)
    assert u is None or tuple(u.shape) == (n_rays, S), (None if u is None else tuple(u.shape), n_rays, S)
    z = torch.empty(n_rays, S, device=ray_dirs.device, dtype=torch.float32)
    pts = torch.empty(n_rays * S, 3, device=ray_dirs.device, dtype=torch.float32)
    fn, ns = _entry(lib, "sc_ray_sample_forward", S)
    code = fn(_lib.ptr(cam_loc), _lib.ptr(ray_dirs), _lib.ptr(scale_dist), _lib.ptr(u), n_rays, *ns, rays_per_image,
              scale_dist.shape[0], cam_dist, _lib.ptr(z), _lib.ptr(pts), _lib.stream())
    _lib.check(code, "sc_ray_sample_forward")
    return z, pts


def ray_sample_forward_eik(cam_loc, ray_dirs, scale_dist, u, eik_idx, eik_uniform, rays_per_image, cam_dist, n_samples=64):
    """ray_sample_forward + the eikonal sample points of the render [B, 2 R, 3] (uniform block | near-surface block) in the same launch."""
    lib = _lib.load()
    n_rays, B = ray_dirs.shape[0], scale_dist.shape[0]
    S = u.shape[1] if u is not None else int(n_samples)
    z = torch.empty(n_rays, S, device=ray_dirs.device, dtype=torch.float32)
    pts = torch.empty(n_rays * S, 3, device=ray_dirs.device, dtype=torch.float32)
    eik = torch.empty(B, 2 * rays_per_image, 3, device=ray_dirs.device, dtype=torch.float32)
    fn, ns = _entry(lib, "sc_ray_sample_forward_eik", S)
    code = fn(_lib.ptr(cam_loc), _lib.ptr(ray_dirs), _lib.ptr(scale_dist), _lib.ptr(u), _lib.ptr(eik_idx), _lib.ptr(eik_uniform),
              n_rays, *ns, rays_per_image, B, cam_dist, _lib.ptr(z), _lib.ptr(pts), _lib.ptr(eik),
              _lib.stream())
    _lib.check(code, "sc_ray_sample_forward_eik")
    return z, pts, eik


def _ray_sample_backward(name, eik, ray_dirs, z_vals, g_points, g_z, rays_per_image, n_images, cam_dist):
    """`eik`: the (eik_idx, g_eik) pair the _eik entry points take after g_z, () for the plain ones."""
    lib = _lib.load()
    n_rays = ray_dirs.shape[0]
    dev = ray_dirs.device
    g_o = torch.empty(n_rays, 3, device=dev, dtype=torch.float32)
    g_d = torch.empty(n_rays, 3, device=dev, dtype=torch.float32)
    g_sd = torch.empty(n_rays, device=dev, dtype=torch.float32)
    fn, ns = _entry(lib, name, z_vals.shape[1])
    code = fn(_lib.ptr(ray_dirs), _lib.ptr(z_vals), _lib.ptr(g_points), _lib.ptr(g_z), *[_lib.ptr(t) for t in eik], n_rays, *ns,
              rays_per_image, n_images, cam_dist, _lib.ptr(g_o), _lib.ptr(g_d), _lib.ptr(g_sd), _lib.stream())
    _lib.check(code, name)
    return g_o, g_d, g_sd.view(n_images, rays_per_image).sum(dim=1)


def ray_sample_backward_eik(ray_dirs, z_vals, g_points, g_z, eik_idx, g_eik, rays_per_image, n_images, cam_dist):
    return _ray_sample_backward("sc_ray_sample_backward_eik", (eik_idx, g_eik), ray_dirs, z_vals, g_points, g_z, rays_per_image, n_images, cam_dist)


def ray_sample_backward(ray_dirs, z_vals, g_points, g_z, rays_per_image, n_images, cam_dist):
    return _ray_sample_backward("sc_ray_sample_backward", (), ray_dirs, z_vals, g_points, g_z, rays_per_image, n_images, cam_dist)


def sdf_grid_forward(w_pack, cbias, lo, hi, n_axis, symmetric=True, split=None):
    """compute_level_grid in one call: -> level [n_images, n_axis, n_axis, n_axis]."""
    lib = _lib.load()
    name = "sc_sdf_grid_forward_split" if (SDF_VALUE_SPLIT if split is None else split) else "sc_sdf_grid_forward"
    B, dev = cbias.shape[0], cbias.device
    ws = torch.empty(B * n_axis ** 3, 3, device=dev, dtype=torch.float32)
    level = torch.empty(B, n_axis, n_axis, n_axis, device=dev, dtype=torch.float32)
    _lib.check(getattr(lib, name)(_lib.ptr(w_pack), _lib.ptr(cbias), lo, hi, n_axis, B, 1 if symmetric else 0, _lib.ptr(ws),
                                  _lib.ptr(level), _lib.stream()), name)
    return level


def render_forward(cam_loc, ray_dirs, depth_fac, scale_dist, u, sdf_pack, sdf_cbias, rgb_pack, rgb_dbias, beta_param,
                   rays_per_image, symmetric, cam_dist, beta_min, bgcolor, normal_pow):
    """One gradient-free render through the single C entry point sc_render_forward."""
    lib = _lib.load()
    n_rays = ray_dirs.shape[0]
    dev = ray_dirs.device
    f32 = dict(device=dev, dtype=torch.float32)
    P = n_rays * 64
    out = dict(rgb=torch.empty(n_rays, 3, **f32), mask=torch.empty(n_rays, **f32), mask_hard=torch.empty(n_rays, **f32),
               depth=torch.empty(n_rays, **f32), normal=torch.empty(n_rays, 3, **f32))
    z = torch.empty(n_rays, 64, **f32); pts = torch.empty(P, 3, **f32); sdf = torch.empty(P, **f32)
    grad = torch.empty(P, 3, **f32); feat = torch.empty(n_tiles(P) * 1024, **f32)
    code = lib.sc_render_forward(
        _lib.ptr(cam_loc), _lib.ptr(ray_dirs), _lib.ptr(depth_fac), _lib.ptr(scale_dist), _lib.ptr(u), _lib.ptr(sdf_pack),
        _lib.ptr(sdf_cbias), _lib.ptr(rgb_pack), _lib.ptr(rgb_dbias), _lib.ptr(beta_param), n_rays, rays_per_image,
        scale_dist.shape[0], 1 if symmetric else 0, cam_dist, beta_min,
        bgcolor, normal_pow, _lib.ptr(out["rgb"]), _lib.ptr(out["mask"]), _lib.ptr(out["mask_hard"]),
        _lib.ptr(out["depth"]), _lib.ptr(out["normal"]), _lib.ptr(z), _lib.ptr(pts), _lib.ptr(sdf), _lib.ptr(grad), _lib.ptr(feat),
        _lib.ptr(_scratch("sdf", dev, SDF_SCRATCH_FLOATS)), None, None, None, _lib.stream())
    _lib.check(code, "sc_render_forward")
    out.update(z_vals=z, points=pts)
    return out


# ---- encoder glue: fused BatchNorm2d (+ residual, ReLU, stem max-pool) -------------------------------------------
# ~270 of these calls per step: the binding is kept lean (plain ints and data_ptr()s through the bound argtypes, no Python frame
# around the ctypes function, one persistent partial-sum buffer per stream).
def _bn_partial(x, groups=1):
    """Workspace for the per-(channel, group) partial sums: at most 2*(2048 + C*G) floats."""
    return _scratch("bn", x.device, max(2 * (2048 + x.shape[1] * groups), 1 << 16)).data_ptr()


def _aligned(t):
    if not t.is_cuda:
        raise RuntimeError(_lib.NO_CPU)
    if not t.is_contiguous():
        t = t.contiguous()
    return t if (t.storage_offset() & 3) == 0 else t.clone()


def _p(t):
    return t.data_ptr() if t is not None else None


def bn_act_forward(x, res, gamma, beta, running_mean, running_var, n_tracked, training, momentum, eps, relu, groups=1):
    """x [N,C,H,W] (+ res) -> y, stats [2,G,C] (save_mean, save_rstd); running statistics updated in place when training."""
    N, C, H, W = x.shape
    y = torch.empty_like(x)
    stats = torch.empty(2, groups, C, device=x.device, dtype=torch.float32)
    sp = stats.data_ptr()
    code = _lib.load().sc_bn_act_forward(x.data_ptr(), _p(res), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), sp,
                                         sp + 4 * C * groups, _p(running_mean), _p(running_var), _p(n_tracked),
                                         _bn_partial(x, groups), N, C, H * W, 1 if relu else 0, 1 if training else 0, groups,
                                         eps, momentum, _lib.raw_stream(x.get_device()))
    if code:
        _lib.check(code, "sc_bn_act_forward")
    return y, stats


def bn_act_backward(dy, x, y, gamma, beta, stats, training, relu, want_dx, want_dres, groups=1):
    N, C, H, W = x.shape
    dx = torch.empty_like(x) if want_dx else None
    dres = torch.empty_like(x) if want_dres else None
    dgb = torch.empty(2, C, device=x.device, dtype=torch.float32)
    sp, gp = stats.data_ptr(), dgb.data_ptr()
    code = _lib.load().sc_bn_act_backward(dy.data_ptr(), x.data_ptr(), _p(y), gamma.data_ptr(), beta.data_ptr(), sp,
                                          sp + 4 * C * groups, _bn_partial(x, groups), _p(dx), _p(dres), gp, gp + 4 * C, N, C,
                                          H * W, 1 if relu else 0, 1 if training else 0, groups, _lib.raw_stream(x.get_device()))
    if code:
        _lib.check(code, "sc_bn_act_backward")
    return dx, dres, dgb[0], dgb[1]


def bn_relu_pool_forward(x, gamma, beta, running_mean, running_var, n_tracked, training, momentum, eps, groups=1):
    N, C, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty(N, C, Ho, Wo, device=x.device, dtype=torch.float32)
    idx = torch.empty(N, C, Ho, Wo, device=x.device, dtype=torch.int32)
    stats = torch.empty(2, groups, C, device=x.device, dtype=torch.float32)
    sp = stats.data_ptr()
    code = _lib.load().sc_bn_relu_pool_forward(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), idx.data_ptr(),
                                               sp, sp + 4 * C * groups, _p(running_mean), _p(running_var), _p(n_tracked),
                                               _bn_partial(x, groups), N, C, H, W, 1 if training else 0, groups, eps, momentum,
                                               _lib.raw_stream(x.get_device()))
    if code:
        _lib.check(code, "sc_bn_relu_pool_forward")
    return y, idx, stats


def bn_relu_pool_backward(dy, idx, x, gamma, beta, stats, training, groups=1):
    N, C, H, W = x.shape
    dx = torch.empty_like(x)
    dgb = torch.empty(2, C, device=x.device, dtype=torch.float32)
    sp, gp = stats.data_ptr(), dgb.data_ptr()
    code = _lib.load().sc_bn_relu_pool_backward(dy.data_ptr(), idx.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                                sp, sp + 4 * C * groups, _bn_partial(x, groups), dx.data_ptr(), gp, gp + 4 * C,
                                                N, C, H, W, 1 if training else 0, groups, _lib.raw_stream(x.get_device()))
    if code:
        _lib.check(code, "sc_bn_relu_pool_backward")
    return dx, dgb[0], dgb[1]


# ---- evaluation: iso-surface triangles of a level grid ---------------------------------------------------------------
ISOSURFACE_METHODS = ("cubes", "tetrahedra")


def isosurface_triangles(level: torch.Tensor, iso: float = 0.0, method: str = "cubes"):
    """level [B,S,S,S] (device) -> (tris [T,3,3] in grid-index units, tri_count [B] int64 on the host).
    method "cubes": marching cubes, the algorithm of the reference's PyMCubes call (same vertex set); "tetrahedra": the
    table-free marching tetrahedra of rounds 1-2.  Count per 1,024-cube block, one scan launch (offsets + per-image totals), one host
    read of the B totals, emit (blocks without a triangle leave at once) -- csrc/isosurface.hip, block form."""
    if method not in ISOSURFACE_METHODS:
        raise ValueError("isosurface_triangles: method must be one of %s, got %r" % (ISOSURFACE_METHODS, method))
    lib = _lib.load()
    count_fn, emit_fn = (lib.sc_marching_cubes_block_count, lib.sc_marching_cubes_block_emit) if method == "cubes" else \
        (lib.sc_isosurface_block_count, lib.sc_isosurface_block_emit)
    level = level.contiguous().float()
    B, S = level.shape[0], level.shape[1]
    assert level.shape[1:] == (S, S, S)
    bpi = int(lib.sc_isosurface_blocks_per_image(S))
    if bpi <= 0:
        raise RuntimeError("shapeclipper_amd: isosurface_triangles needs 2 <= grid side <= 1024, got %d" % S)
    counts = torch.empty(B * bpi, device=level.device, dtype=torch.int32)           # triangles per workgroup of 1,024 cubes
    masks = None
    if method == "cubes":       # the case index of every cube goes from the count pass to the emit pass (1 byte per cube)
        masks = torch.empty(B * (S - 1) ** 3, device=level.device, dtype=torch.uint8)
        _lib.check(lib.sc_marching_cubes_block_count_masks(_lib.ptr(level), B, S, iso, _lib.ptr(counts), _lib.ptr(masks),
                                                           _lib.stream()), "sc_marching_cubes_block_count_masks")
    else:
        _lib.check(count_fn(_lib.ptr(level), B, S, iso, _lib.ptr(counts), _lib.stream()), "sc_isosurface_block_count")
    offsets = torch.empty(B * bpi + 1, device=level.device, dtype=torch.int64)      # exclusive prefix, the total last
    per_image = torch.empty(B, device=level.device, dtype=torch.int64)
    _lib.check(lib.sc_isosurface_block_scan(_lib.ptr(counts), B, S, _lib.ptr(offsets), _lib.ptr(per_image), _lib.stream()),
               "sc_isosurface_block_scan")
    per_image = per_image.cpu()                                                       # the one host read: it sizes the output
    total = int(per_image.sum())
    tris = torch.empty(total, 3, 3, device=level.device, dtype=torch.float32)
    if total > 0 and masks is not None:
        _lib.check(lib.sc_marching_cubes_block_emit_masks(_lib.ptr(level), B, S, iso, _lib.ptr(offsets), _lib.ptr(masks),
                                                          _lib.ptr(tris), _lib.stream()), "sc_marching_cubes_block_emit_masks")
    elif total > 0:
        _lib.check(emit_fn(_lib.ptr(level), B, S, iso, _lib.ptr(offsets), _lib.ptr(tris), _lib.stream()),
                   "sc_isosurface_block_emit / sc_marching_cubes_block_emit")
    return tris, per_image


_MeshState = collections.namedtuple("_MeshState", ["level", "masks", "offsets", "voffsets", "verts", "vmap", "v_count", "f_count"])


def _mesh_state(level, iso, who):
    """What the indexed marching-cubes mesh and the dual mesh share, up to and including the vertex emit: the contiguous fp32 grid, the
    case byte of every cube, the triangle block offsets, the vertex block offsets, the crossing vertices verts [V,3] (grid-index units),
    the vertex-number map (None when V == 0) and the two per-image counts on the host.  `who` names the caller in the refusals."""
    lib = _lib.load()
    level = level.contiguous().float()
    B, S = level.shape[0], level.shape[1]
    assert level.shape[1:] == (S, S, S)
    bpi = int(lib.sc_isosurface_blocks_per_image(S))
    vbpi = int(lib.sc_marching_cubes_mesh_vertex_blocks_per_image(S))
    if bpi <= 0 or vbpi <= 0:
        raise RuntimeError("shapeclipper_amd: %s needs 2 <= grid side <= 1024, got %d" % (who, S))
    dev = level.device
    counts = torch.empty(B * bpi, device=dev, dtype=torch.int32)                    # triangles per workgroup of 1,024 cubes
    masks = torch.empty(B * (S - 1) ** 3, device=dev, dtype=torch.uint8)            # case index per cube
    _lib.check(lib.sc_marching_cubes_block_count_masks(_lib.ptr(level), B, S, iso, _lib.ptr(counts), _lib.ptr(masks),
                                                       _lib.stream()), "sc_marching_cubes_block_count_masks")
    offsets = torch.empty(B * bpi + 1, device=dev, dtype=torch.int64)
    f_count = torch.empty(B, device=dev, dtype=torch.int64)
    _lib.check(lib.sc_isosurface_block_scan(_lib.ptr(counts), B, S, _lib.ptr(offsets), _lib.ptr(f_count), _lib.stream()),
               "sc_isosurface_block_scan")
    vcounts = torch.empty(B * vbpi, device=dev, dtype=torch.int32)                  # crossing edges per workgroup of 1,024 grid points
    _lib.check(lib.sc_marching_cubes_mesh_vertex_count(_lib.ptr(level), B, S, iso, _lib.ptr(vcounts), _lib.stream()),
               "sc_marching_cubes_mesh_vertex_count")
    voffsets = torch.empty(B * vbpi + 1, device=dev, dtype=torch.int64)
    v_count = torch.empty(B, device=dev, dtype=torch.int64)
    _lib.check(lib.sc_marching_cubes_mesh_vertex_scan(_lib.ptr(vcounts), B, S, _lib.ptr(voffsets), _lib.ptr(v_count), _lib.stream()),
               "sc_marching_cubes_mesh_vertex_scan")
    counts_host = torch.stack([v_count, f_count]).cpu()                             # the one host read: it sizes both outputs
    v_count, f_count = counts_host[0], counts_host[1]
    if B and int(v_count.max()) > 2 ** 31 - 1:
        raise RuntimeError("shapeclipper_amd: %s: image %d has %d vertices; int32 face indices hold at most 2^31 - 1"
                           % (who, int(v_count.argmax()), int(v_count.max())))
    V = int(v_count.sum())
    verts = torch.empty(V, 3, device=dev, dtype=torch.float32)
    vmap = None
    if V > 0:
        vmap = torch.empty(B * S ** 3 * 3, device=dev, dtype=torch.int32)          # vertex number per (grid point, axis); no fill
        _lib.check(lib.sc_marching_cubes_mesh_vertex_emit(_lib.ptr(level), B, S, iso, _lib.ptr(voffsets), _lib.ptr(verts),
                                                          _lib.ptr(vmap), _lib.stream()), "sc_marching_cubes_mesh_vertex_emit")
    return _MeshState(level, masks, offsets, voffsets, verts, vmap, v_count, f_count)


def isosurface_mesh(level: torch.Tensor, iso: float = 0.0):
    """level [B,S,S,S] (device) -> PackedMesh (mesh_pack.py) with verts in grid-index units and the counts as int64 on the host.

    The indexed form of isosurface_triangles(method="cubes"): one vertex per grid edge whose end values lie on different sides of iso,
    ordered by image, owning grid point (its lower end, linear index) and axis, shared by every triangle around the edge.
    verts[faces] of an image equals its triangles from isosurface_triangles bit for bit, in the same order.  Two scans with one host
    read each (faces: the soup's count / scan over 1,024-cube blocks; vertices: 1,024-point blocks), vertex emit, face emit --
    csrc/isosurface.hip.  Scratch: a vertex-number map of 12 bytes per grid point, written at crossing edges only."""
    st = _mesh_state(level, iso, "isosurface_mesh")
    B, S = st.level.shape[0], st.level.shape[1]
    F = int(st.f_count.sum())
    faces = torch.empty(F, 3, device=st.level.device, dtype=torch.int32)
    if st.vmap is not None and F > 0:
        _lib.check(_lib.load().sc_marching_cubes_mesh_face_emit(B, S, _lib.ptr(st.offsets), _lib.ptr(st.masks), _lib.ptr(st.vmap),
                                                                _lib.ptr(faces), _lib.stream()), "sc_marching_cubes_mesh_face_emit")
    return PackedMesh(st.verts, faces, st.v_count, st.f_count)


def dual_contour_mesh(level: torch.Tensor, normals: torch.Tensor, iso: float = 0.0, reg: float = 0.05):
    """level [B,S,S,S] (device), normals [V,3] fp32 (device) -> PackedMesh (verts in grid-index units, the counts as int64 on the host):
    the dual-contouring mesh of the grid.

    normals belong to the vertices of isosurface_mesh(level, iso), in their order (V of them).  One vertex per cell whose corners lie
    on both sides of iso, where the tangent planes of the cell's crossings meet: the minimiser of sum (n_i . (x - p_i))^2 +
    reg k |x - c|^2 over the cell's k crossings (c their mean), clamped into the cell; per image in ascending cell index.  One quad
    (two triangles) per crossing grid edge with four cells around it, in the order of the crossing vertices, oriented as the faces
    of isosurface_mesh; indices are local to the image.  include/shapeclipper_hip.h states the arithmetic operation by operation
    (csrc/dual_contour.hip; bit-reproducible, no atomics).  On top of isosurface_mesh's launches: count, two scans, one more host read
    to size the outputs, cell emit, face emit.  Scratch: the cell-to-vertex map, 4 bytes per cube, in the scratch cache ("dual contour").
    ValueError for normals that are not fp32 [*,3] on level's device or a reg that is not a finite number > 0, before any launch, and
    for a row count other than V once the crossing vertices are counted (before any dual-contouring launch); isosurface_mesh's refusals
    otherwise."""
    reg = float(reg)
    if not 0.0 < reg < float("inf"):
        raise ValueError("shapeclipper_amd: dual_contour_mesh needs a finite reg > 0, got %r" % reg)
    if not isinstance(normals, torch.Tensor) or normals.dtype != torch.float32 or normals.dim() != 2 or normals.shape[1] != 3:
        raise ValueError("shapeclipper_amd: dual_contour_mesh takes normals [V,3] fp32, got %s" % (
            "%s %s" % (tuple(normals.shape), normals.dtype) if isinstance(normals, torch.Tensor) else type(normals).__name__))
    if normals.device != level.device:
        raise ValueError("shapeclipper_amd: dual_contour_mesh: normals on %s, level on %s" % (normals.device, level.device))
    lib = _lib.load()
    st = _mesh_state(level, iso, "dual_contour_mesh")
    B, S = st.level.shape[0], st.level.shape[1]
    dev = st.level.device
    if normals.shape[0] != st.verts.shape[0]:
        raise ValueError("shapeclipper_amd: dual_contour_mesh: %d normals for the %d crossing vertices of isosurface_mesh(level, iso)"
                         % (normals.shape[0], st.verts.shape[0]))
    if st.vmap is None:                                                             # no crossing edge: no image has a surface
        return PackedMesh.empty(B, dev)
    normals = normals.contiguous()
    bpi = int(lib.sc_isosurface_blocks_per_image(S))
    counts = torch.empty(2, B * bpi, device=dev, dtype=torch.int32)                 # owning cells / triangles per 1,024-cube block
    _lib.check(lib.sc_dual_contour_count(_lib.ptr(st.masks), B, S, _lib.ptr(counts[0]), _lib.ptr(counts[1]), _lib.stream()),
               "sc_dual_contour_count")
    offsets = torch.empty(2, B * bpi + 1, device=dev, dtype=torch.int64)
    totals = torch.empty(2, B, device=dev, dtype=torch.int64)
    for k in range(2):
        _lib.check(lib.sc_isosurface_block_scan(_lib.ptr(counts[k]), B, S, _lib.ptr(offsets[k]), _lib.ptr(totals[k]), _lib.stream()),
                   "sc_isosurface_block_scan")
    totals = totals.cpu()                                                           # the one host read: it sizes both outputs
    v_count, f_count = totals[0], totals[1]
    Vd, Fd = int(v_count.sum()), int(f_count.sum())
    verts = torch.empty(Vd, 3, device=dev, dtype=torch.float32)
    faces = torch.empty(Fd, 3, device=dev, dtype=torch.int32)
    cell_map = _scratch("dual contour", dev, B * (S - 1) ** 3).view(torch.int32)   # dual vertex number per cube; written at owning cells only
    _lib.check(lib.sc_dual_contour_cell_emit(_lib.ptr(st.masks), _lib.ptr(st.verts), _lib.ptr(normals), _lib.ptr(st.vmap),
                                             _lib.ptr(st.voffsets), B, S, reg, _lib.ptr(offsets[0]), _lib.ptr(verts), _lib.ptr(cell_map),
                                             _lib.stream()), "sc_dual_contour_cell_emit")
    if Fd > 0:
        _lib.check(lib.sc_dual_contour_face_emit(_lib.ptr(st.masks), _lib.ptr(cell_map), B, S, _lib.ptr(offsets[1]), _lib.ptr(faces),
                                                 _lib.stream()), "sc_dual_contour_face_emit")
    return PackedMesh(verts, faces, v_count, f_count)


# ---- evaluation: the largest connected component of a level grid's solid (csrc/level_components.hip) -------------------------------
LEVEL_COMPONENTS_MAX_IMAGES = 65535
ComponentStats = collections.namedtuple("ComponentStats", ["n_components", "inside_voxels", "kept_voxels"])


def level_largest_component(level: torch.Tensor, iso: float = 0.0):
    """level [B,S,S,S] fp32 (device) -> (level_out [B,S,S,S], ComponentStats of int32 [B] tensors n_components, inside_voxels, kept_voxels).

    The inside voxels (level < iso; NaN is outside) of each image fall into components under 6-connectivity; the largest one is kept,
    among equals the one whose smallest linear index (x S + y) S + z is smallest.  level_out holds level's bits except at the inside voxels
    of the other components, which hold iso + (iso - level), outside.  sc_level_largest_component (include/shapeclipper_hip.h states the
    definition): integer atomics only, bit-reproducible, no host synchronisation; its labels live in the "level components" buffer of
    the scratch cache.  ValueError for a grid that is not [B,S,S,S], not fp32, S outside 2..1024 or B > 65535."""
    if level.dim() != 4 or not (level.shape[1] == level.shape[2] == level.shape[3]):
        raise ValueError("shapeclipper_amd: level_largest_component takes a cubic grid [B,S,S,S], got shape %s" % (tuple(level.shape),))
    if level.dtype != torch.float32:
        raise ValueError("shapeclipper_amd: level_largest_component takes an fp32 grid, got %s" % level.dtype)
    B, S = level.shape[0], level.shape[1]
    if not 2 <= S <= 1024:
        raise ValueError("shapeclipper_amd: level_largest_component needs 2 <= grid side <= 1024, got %d" % S)
    if B > LEVEL_COMPONENTS_MAX_IMAGES:
        raise ValueError("shapeclipper_amd: level_largest_component takes at most %d images per call, got %d" % (LEVEL_COMPONENTS_MAX_IMAGES, B))
    if not level.is_cuda:
        raise RuntimeError(_lib.NO_CPU)
    lib = _lib.load()
    level = level.contiguous()
    out = torch.empty_like(level)
    stats = torch.empty(3, B, device=level.device, dtype=torch.int32)
    if B > 0:
        ws = _scratch("level components", level.device, (lib.sc_level_largest_component_scratch_bytes(B, S) + 3) // 4)
        code = lib.sc_level_largest_component(_lib.ptr(level), B, S, float(iso), _lib.ptr(out), _lib.ptr(stats[0]), _lib.ptr(stats[1]),
                                              _lib.ptr(stats[2]), _lib.ptr(ws), _lib.stream())
        _lib.check(code, "sc_level_largest_component")
    return out, ComponentStats(stats[0], stats[1], stats[2])

# ---- surface render: the per-ray root finder (csrc/surface_hit.hip) -----------------------------------------------------------------
SURFACE_HIT_MAX_RAYS = 1 << 30          # SC_SURFACE_HIT_MAX_RAYS (include/shapeclipper_hip.h)
RayBracket = collections.namedtuple("RayBracket", ["t_lo", "t_hi", "f_lo", "f_hi", "hit"])


def _surface_arg(name, t, shape, dtype=torch.float32):
    """ValueError unless t is a device tensor of this dtype and shape (the two surface ops refuse everything else before any launch)."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise ValueError("shapeclipper_amd: %s must be a %s tensor of shape %s, got %s" % (
            name, str(dtype).replace("torch.", ""), tuple(shape), "%s %s" % (tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__))
    if not t.is_cuda:
        raise ValueError(_lib.NO_CPU)
    return t.contiguous()


def ray_first_crossing(z_vals: torch.Tensor, sdf: torch.Tensor, iso: float = 0.0) -> RayBracket:
    """z_vals [n_rays,S], sdf [n_rays*S] fp32 (device; sample i of ray r at r S + i, the layout of sdf_forward on ray_sample_forward's
    points) -> RayBracket(t_lo, t_hi, f_lo, f_hi fp32 [n_rays], hit int32 [n_rays]).

    With f_i = sdf_i - iso: hit 2 where f_0 <= 0 (the ray starts inside; bracket = sample 0 twice), else hit 1 at the first pair with
    f_i > 0 and f_{i+1} <= 0 (bracket = that pair), else hit 0 (bracket = sample 0 twice).  sc_ray_first_crossing
    (include/shapeclipper_hip.h states the definition): no atomics, no scratch, no host synchronisation.  ValueError for CPU tensors,
    another dtype or shape, or an S outside sample_count_supported."""
    if not isinstance(z_vals, torch.Tensor) or z_vals.dim() != 2:
        raise ValueError("shapeclipper_amd: ray_first_crossing takes z_vals [n_rays,S], got %s" % (tuple(z_vals.shape) if isinstance(z_vals, torch.Tensor) else type(z_vals).__name__,))
    n, S = z_vals.shape
    if not sample_count_supported(S):
        raise ValueError("shapeclipper_amd: ray_first_crossing takes S %% 32 == 0, 32 <= S <= 256 samples per ray, not %d" % S)
    if n > SURFACE_HIT_MAX_RAYS:
        raise ValueError("shapeclipper_amd: ray_first_crossing takes at most %d rays per call, got %d" % (SURFACE_HIT_MAX_RAYS, n))
    z_vals = _surface_arg("z_vals", z_vals, (n, S))
    sdf = _surface_arg("sdf", sdf, (n * S,))
    lib = _lib.load()
    f = torch.empty(4, n, device=z_vals.device, dtype=torch.float32)
    hit = torch.empty(n, device=z_vals.device, dtype=torch.int32)
    code = lib.sc_ray_first_crossing(_lib.ptr(z_vals), _lib.ptr(sdf), n, S, float(iso), _lib.ptr(f[0]), _lib.ptr(f[1]), _lib.ptr(f[2]),
                                     _lib.ptr(f[3]), _lib.ptr(hit), _lib.stream())
    _lib.check(code, "sc_ray_first_crossing")
    return RayBracket(f[0], f[1], f[2], f[3], hit)


def ray_bracket_step(bracket: RayBracket, cam_loc: torch.Tensor, ray_dirs: torch.Tensor, f_new: torch.Tensor = None,
                     t_prev: torch.Tensor = None, iso: float = 0.0):
    """One step of the safeguarded regula falsi on every ray -> (t [n_rays], points [n_rays,3] = cam_loc + t * ray_dirs).

    bracket: a RayBracket of contiguous tensors, UPDATED IN PLACE on its hit == 1 rays when f_new is given: f_new [n_rays] is the SDF at
    the previous query t_prev [n_rays] (the t this function returned last); f_new - iso > 0 moves the lower end there, <= 0 the upper
    end, NaN nothing.  Then the query: t_lo + w (t_hi - t_lo) with w = f_lo / (f_lo - f_hi), w = 0.5 when that is not a number in
    [0, 1] or the difference overflowed, clamped to the bracket; t_lo on rays with hit != 1.  cam_loc, ray_dirs [n_rays,3] as
    camera_rays_forward returns them.  sc_ray_bracket_step (include/shapeclipper_hip.h): one launch, no scratch, no host
    synchronisation.  ValueError for CPU tensors, another dtype or shape, or f_new without t_prev."""
    if not isinstance(bracket, RayBracket) or not isinstance(bracket.hit, torch.Tensor) or bracket.hit.dim() != 1:
        raise ValueError("shapeclipper_amd: ray_bracket_step takes the RayBracket of ray_first_crossing")
    n = bracket.hit.shape[0]
    if n > SURFACE_HIT_MAX_RAYS:
        raise ValueError("shapeclipper_amd: ray_bracket_step takes at most %d rays per call, got %d" % (SURFACE_HIT_MAX_RAYS, n))
    for name, x in zip(RayBracket._fields, bracket):
        _surface_arg("bracket.%s" % name, x, (n,), torch.int32 if name == "hit" else torch.float32)
        if not x.is_contiguous():
            raise ValueError("shapeclipper_amd: bracket.%s must be contiguous (it is updated in place)" % name)
    cam_loc = _surface_arg("cam_loc", cam_loc, (n, 3))
    ray_dirs = _surface_arg("ray_dirs", ray_dirs, (n, 3))
    if (f_new is None) != (t_prev is None):
        raise ValueError("shapeclipper_amd: ray_bracket_step takes f_new and t_prev together (the SDF value at the previous query)")
    if f_new is not None:
        f_new, t_prev = _surface_arg("f_new", f_new, (n,)), _surface_arg("t_prev", t_prev, (n,))
    lib = _lib.load()
    t = torch.empty(n, device=cam_loc.device, dtype=torch.float32)
    points = torch.empty(n, 3, device=cam_loc.device, dtype=torch.float32)
    code = lib.sc_ray_bracket_step(_lib.ptr(cam_loc), _lib.ptr(ray_dirs), _lib.ptr(f_new), _lib.ptr(t_prev), n, float(iso),
                                   _lib.ptr(bracket.t_lo), _lib.ptr(bracket.t_hi), _lib.ptr(bracket.f_lo), _lib.ptr(bracket.f_hi),
                                   _lib.ptr(bracket.hit), _lib.ptr(t), _lib.ptr(points), _lib.stream())
    _lib.check(code, "sc_ray_bracket_step")
    return t, points


# ---- camera algebra ------------------------------------------------------------------------------------------------
def camera_rays_forward(pose, intr, ray_idx, n_rays, width):
    lib = _lib.load()
    B = pose.shape[0]
    f32 = dict(device=pose.device, dtype=torch.float32)
    cam_loc = torch.empty(B * n_rays, 3, **f32)
    dirs = torch.empty(B * n_rays, 3, **f32)
    depth_fac = torch.empty(B * n_rays, **f32)
    _lib.check(lib.sc_camera_rays_forward(_lib.ptr(pose), _lib.ptr(intr), _lib.ptr(ray_idx), B, n_rays, width,
                                          _lib.ptr(cam_loc), _lib.ptr(dirs), _lib.ptr(depth_fac), _lib.stream()),
               "sc_camera_rays_forward")
    return cam_loc, dirs, depth_fac


def camera_rays_backward(pose, intr, ray_idx, n_rays, width, g_cam_loc, g_dirs, g_depth_fac):
    lib = _lib.load()
    B = pose.shape[0]
    g_pose, g_intr = torch.empty_like(pose), torch.empty_like(intr)
    _lib.check(lib.sc_camera_rays_backward(_lib.ptr(pose), _lib.ptr(intr), _lib.ptr(ray_idx), B, n_rays, width,
                                           _lib.ptr(g_cam_loc), _lib.ptr(g_dirs), _lib.ptr(g_depth_fac), _lib.ptr(g_pose),
                                           _lib.ptr(g_intr), _lib.stream()), "sc_camera_rays_backward")
    return g_pose, g_intr


def pose_from_trig_forward(azim, elev, theta, scale_focal, scale_dist, cam_dist, focal, width, height):
    lib = _lib.load()
    B = azim.shape[0]
    pose = torch.empty(B, 3, 4, device=azim.device, dtype=torch.float32)
    intr = torch.empty(B, 3, 3, device=azim.device, dtype=torch.float32)
    _lib.check(lib.sc_pose_from_trig_forward(_lib.ptr(azim), _lib.ptr(elev), _lib.ptr(theta), _lib.ptr(scale_focal),
                                             _lib.ptr(scale_dist), B, cam_dist, focal,
                                             width, height, _lib.ptr(pose), _lib.ptr(intr), _lib.stream()),
               "sc_pose_from_trig_forward")
    return pose, intr


def pose_from_trig_backward(azim, elev, theta, scale_focal, scale_dist, cam_dist, focal, width, height, g_pose, g_intr):
    lib = _lib.load()
    B = azim.shape[0]
    g = torch.empty(8, B, device=azim.device, dtype=torch.float32)      # azim[B,2] | elev[B,2] | theta[B,2] | sf[B] | sd[B]
    ga, ge, gt = g[0:2].view(B, 2), g[2:4].view(B, 2), g[4:6].view(B, 2)
    _lib.check(lib.sc_pose_from_trig_backward(_lib.ptr(azim), _lib.ptr(elev), _lib.ptr(theta), _lib.ptr(scale_focal),
                                              _lib.ptr(scale_dist), B, cam_dist, focal,
                                              width, height, _lib.ptr(g_pose), _lib.ptr(g_intr), _lib.ptr(ga),
                                              _lib.ptr(ge), _lib.ptr(gt), _lib.ptr(g[6]), _lib.ptr(g[7]), _lib.stream()),
               "sc_pose_from_trig_backward")
    return ga, ge, gt, g[6], g[7]


# ---------------------------------------------------------------------------------------------------------------------------
# the [B]-sized arithmetic around the view estimator (csrc/camera_prior.hip)
def _ptr_array(tensors):
    """HOST array of device pointers (NULL for None) for the entry points that take `const float* const*`."""
    return (ctypes.c_void_p * max(len(tensors), 1))(*[_lib.ptr(t).value for t in tensors])


def _f32c(t):
    if t is not None and not (t.is_contiguous() and t.dtype == torch.float32):
        t = t.contiguous().float()
    return t


def estimator_head_forward(trig, size_lin, persp_lin, size_range, persp_range):
    """trig [N,6], size_lin, persp_lin [N] -> one [8, N] buffer holding azim [N,2] | elev [N,2] | theta [N,2] | scale_focal [N] | scale_dist [N]."""
    lib = _lib.load()
    N = trig.shape[0]
    o = torch.empty(8 * N, device=trig.device, dtype=torch.float32)
    _lib.check(lib.sc_estimator_head_forward(_lib.ptr(trig), _lib.ptr(size_lin), _lib.ptr(persp_lin), N, size_range,
                                             persp_range, _lib.ptr(o[0:2 * N]), _lib.ptr(o[2 * N:4 * N]), _lib.ptr(o[4 * N:6 * N]),
                                             _lib.ptr(o[6 * N:7 * N]), _lib.ptr(o[7 * N:8 * N]), _lib.stream()), "sc_estimator_head_forward")
    return o


def estimator_head_backward(trig, size_lin, persp_lin, size_range, persp_range, grads, n_groups):
    """grads: 5 * n_groups upstream gradients (None = not differentiated), group-major."""
    lib = _lib.load()
    N = trig.shape[0]
    g = torch.empty(8 * N, device=trig.device, dtype=torch.float32)
    grads = [_f32c(t) for t in grads]
    _lib.check(lib.sc_estimator_head_backward(_lib.ptr(trig), _lib.ptr(size_lin), _lib.ptr(persp_lin), N, size_range,
                                              persp_range, _ptr_array(grads), n_groups, _lib.ptr(g[:6 * N]),
                                              _lib.ptr(g[6 * N:7 * N]), _lib.ptr(g[7 * N:]), _lib.stream()), "sc_estimator_head_backward")
    return g[:6 * N].view(N, 6), g[6 * N:7 * N], g[7 * N:]


_PRIOR_MAX = None


def camera_prior_supported(n_images, emd_p) -> bool:
    global _PRIOR_MAX
    if _PRIOR_MAX is None:
        _PRIOR_MAX = int(_lib.load().sc_camera_prior_max_images())
    return 0 < n_images <= _PRIOR_MAX and emd_p in (1, 2)


def camera_prior_forward(azim, elev, theta, f_azim, f_elev, f_theta, elev_range, theta_range, margin_eps, emd_p):
    """-> out [3] (cam_margin, cam_uniform, cam_sym), grads [6, B, 2] (see include/shapeclipper_hip.h)."""
    lib = _lib.load()
    B = azim.shape[0]
    out = torch.empty(3, device=azim.device, dtype=torch.float32)
    grads = torch.empty(6, B, 2, device=azim.device, dtype=torch.float32)
    _lib.check(lib.sc_camera_prior_forward(_lib.ptr(azim), _lib.ptr(elev), _lib.ptr(theta), _lib.ptr(f_azim), _lib.ptr(f_elev),
                                           _lib.ptr(f_theta), B, elev_range[0], elev_range[1],
                                           theta_range[0], theta_range[1], margin_eps, emd_p,
                                           _lib.ptr(out), _lib.ptr(grads), _lib.stream()), "sc_camera_prior_forward")
    return out, grads


def camera_prior_backward(grads, G_margin, G_uniform, G_sym):
    """-> g [6, B, 2]: azim, elev, theta, flipped azim, flipped elev, flipped theta."""
    lib = _lib.load()
    B = grads.shape[1]
    g = torch.empty(6, B, 2, device=grads.device, dtype=torch.float32)
    _lib.check(lib.sc_camera_prior_backward(_lib.ptr(grads), B, _lib.ptr(_f32c(G_margin)), _lib.ptr(_f32c(G_uniform)),
                                            _lib.ptr(_f32c(G_sym)), *[_lib.ptr(g[k]) for k in range(6)], _lib.stream()),
               "sc_camera_prior_backward")
    return g


def transform_normal_forward(normals, pose):
    lib = _lib.load()
    B, R = normals.shape[0], normals.shape[1]
    out = torch.empty(B, R, 3, device=normals.device, dtype=torch.float32)
    _lib.check(lib.sc_transform_normal_forward(_lib.ptr(normals), _lib.ptr(pose), B, R, _lib.ptr(out), _lib.stream()),
               "sc_transform_normal_forward")
    return out


def transform_normal_backward(normals, g_out):
    lib = _lib.load()
    B, R = normals.shape[0], normals.shape[1]
    g_pose = torch.empty(B, 3, 4, device=normals.device, dtype=torch.float32)
    _lib.check(lib.sc_transform_normal_backward(_lib.ptr(normals), _lib.ptr(g_out), B, R, _lib.ptr(g_pose), _lib.stream()),
               "sc_transform_normal_backward")
    return g_pose


LOSS_TOTAL_MAX_TERMS = 16


def loss_total_forward(values, weights):
    """values: device scalars, weights: python floats -> (total [], bad [] bool)."""
    lib = _lib.load()
    dev = values[0].device
    total = torch.empty((), device=dev, dtype=torch.float32)
    bad = torch.empty((), device=dev, dtype=torch.bool)
    w = (ctypes.c_float * len(weights))(*weights)
    _lib.check(lib.sc_loss_total_forward(_ptr_array(values), w, len(values), _lib.ptr(total), _lib.ptr(bad), _lib.stream()),
               "sc_loss_total_forward")
    return total, bad


def loss_total_backward(weights, G):
    lib = _lib.load()
    g = torch.empty(len(weights), device=G.device, dtype=torch.float32)
    w = (ctypes.c_float * len(weights))(*weights)
    _lib.check(lib.sc_loss_total_backward(w, len(weights), _lib.ptr(_f32c(G)), _lib.ptr(g), _lib.stream()), "sc_loss_total_backward")
    return g


# ---------------------------------------------------------------------------------------------------------------------------
# 3x3 stride-1 convolutions of the ResNet trunks on the fp32 matrix pipe (csrc/conv3x3.hip)
CONV3X3_SIDES = (56, 28, 14, 7)


def conv3x3_supported(x_shape, w_shape, stride=1, padding=1) -> bool:
    """Shapes sc_conv3x3_forward takes: square 56/28/14/7 maps, 3x3 filter, stride 1, pad 1, channel counts that are multiples of 8."""
    return (len(x_shape) == 4 and tuple(w_shape[2:]) == (3, 3) and stride in (1, (1, 1)) and padding in (1, (1, 1))
            and x_shape[2] == x_shape[3] and x_shape[2] in CONV3X3_SIDES and w_shape[1] == x_shape[1]
            and w_shape[0] % 8 == 0 and w_shape[1] % 8 == 0)


def conv3x3_pack(w, side, transpose_flip=False, split=False):
    """Kernel-ready weight image of w [Cout, Cin, 3, 3] for `side` x `side` maps (transpose_flip: the backward-data filter;
    split: the three-piece bf16 image of sc_conv3x3_forward_split)."""
    lib = _lib.load()
    w = _aligned(w)
    cin, cout = (w.shape[0], w.shape[1]) if transpose_flip else (w.shape[1], w.shape[0])
    n = (lib.sc_conv3x3_pack_floats_split if split else lib.sc_conv3x3_pack_floats)(cin, cout, side)
    if n < 0:
        raise RuntimeError("shapeclipper_amd: sc_conv3x3 does not take %dx%d maps with a %s filter" % (side, side, tuple(w.shape)))
    w_pack = torch.empty(n, device=w.device, dtype=torch.float32)
    _lib.check(lib.sc_conv3x3_pack(_lib.ptr(w), _lib.ptr(w_pack), cin, cout, side, int(transpose_flip) | (2 if split else 0), _lib.stream()),
               "sc_conv3x3_pack")
    return w_pack


def set_reserved_cus(n: int) -> int:
    """Size the persistent convolution grids for (device CUs - n) compute units (sc_set_reserved_cus; `--hip.reserve_cus`): leaves n CUs
    to concurrently running kernels of other streams (RCCL's all-reduce in a multi-GPU step).  Returns the resulting grid size.  The cached
    partial-tile workspaces are dropped when the value changes (their sizes follow the grid)."""
    lib = _lib.load()
    before = lib.sc_grid_cus()
    _lib.check(lib.sc_set_reserved_cus(int(n)), "sc_set_reserved_cus")
    after = lib.sc_grid_cus()
    if after != before:
        for key in [k for k in _SCRATCH if k[0].startswith("conv")]:
            del _SCRATCH[key]
    return after


def _conv_workspace(dev, side, split=False):
    """Scratch for the partial tiles of sc_conv3x3_forward, one per (device, stream, map side, arithmetic)."""
    lib = _lib.load()
    n = (lib.sc_conv3x3_workspace_floats_split if split else lib.sc_conv3x3_workspace_floats)(side)
    return _scratch("conv3x3 %d %d" % (side, split), dev, n)


def conv3x3_apply(x, w_pack, cout, split=False):
    lib = _lib.load()
    x = _aligned(x)
    B, cin, H, _ = x.shape
    out = torch.empty(B, cout, H, H, device=x.device, dtype=torch.float32)
    fn = lib.sc_conv3x3_forward_split if split else lib.sc_conv3x3_forward
    _lib.check(fn(_lib.ptr(x), _lib.ptr(w_pack), _lib.ptr(out), _lib.ptr(_conv_workspace(x.device, H, split)), B, cin, cout, H, _lib.stream()),
               "sc_conv3x3_forward")
    return out


def _conv3x3(x, w, transpose_flip, split=False):
    if x.dim() != 4 or x.shape[2] != x.shape[3]:
        raise RuntimeError("shapeclipper_amd: sc_conv3x3 needs square NCHW maps, got %s" % (tuple(x.shape),))
    return conv3x3_apply(x, conv3x3_pack(w, x.shape[2], transpose_flip, split), w.shape[1] if transpose_flip else w.shape[0], split)


def conv3x3_forward(x, w, split=False):
    """F.conv2d(x, w, None, 1, 1) for x [B, Cin, H, H], w [Cout, Cin, 3, 3].  split: fp32-accurate products on the bf16 matrix pipe."""
    return _conv3x3(x, w, False, split)


def conv3x3_backward_data(gy, w, split=False):
    """dL/dx of the above from gy [B, Cout, H, H]: the same kernel with the transposed, flipped filter."""
    return _conv3x3(gy, w, True, split)


def conv3x3_wgrad_supported(x_shape, w_shape, stride=1, padding=1) -> bool:
    return conv3x3_supported(x_shape, w_shape, stride, padding) and w_shape[0] % 64 == 0 and w_shape[1] % 64 == 0


def conv3x3_backward_weight(gy, x, split=False):
    """dL/dw [Cout, Cin, 3, 3] of F.conv2d(x, w, None, 1, 1) from gy [B, Cout, H, H] and x [B, Cin, H, H] (sc_conv3x3_wgrad).
    split: fp32-accurate products on the bf16 matrix pipe (sc_conv3x3_wgrad_split), the arithmetic of the split forward pass."""
    lib = _lib.load()
    gy, x = _aligned(gy), _aligned(x)
    B, cout, H, _ = gy.shape
    cin = x.shape[1]
    n = lib.sc_conv3x3_wgrad_workspace_floats(cin, cout)
    if n < 0 or H not in CONV3X3_SIDES or x.shape[0] != B or tuple(x.shape[2:]) != (H, H):
        raise RuntimeError("shapeclipper_amd: sc_conv3x3_wgrad does not take gy %s with x %s" % (tuple(gy.shape), tuple(x.shape)))
    ws = _scratch("conv wgrad", x.device, n)
    dw = torch.empty(cout, cin, 3, 3, device=x.device, dtype=torch.float32)
    fn = lib.sc_conv3x3_wgrad_split if split else lib.sc_conv3x3_wgrad
    _lib.check(fn(_lib.ptr(gy), _lib.ptr(x), _lib.ptr(dw), _lib.ptr(ws), B, cin, cout, H, _lib.stream()), "sc_conv3x3_wgrad")
    return dw


# ---- one C call per BasicBlock (csrc/block.hip; include/shapeclipper_hip.h: sc_block_args) ---------------------------------------------
class BlockArgs(ctypes.Structure):
    """ctypes mirror of sc_block_args (field order and types of include/shapeclipper_hip.h)."""
    _fields_ = ([(n, ctypes.c_void_p) for n in ("x", "pf1", "pf2", "pb1", "pb2", "g1", "b1", "g2", "b2", "rm1", "rv1", "rm2", "rv2", "nt1", "nt2",
                                   "y1", "a1", "y2", "out", "st1", "st2", "conv_ws", "bn_ws", "wgrad_ws", "d_out",
                                   "dy2", "dres", "da1", "dy1", "dx", "gw1", "gw2", "dgb1", "dgb2")]
                + [(n, ctypes.c_int) for n in ("batch", "channels", "hw", "groups", "training", "split", "need_dx")]
                + [(n, ctypes.c_float) for n in ("mom1", "eps1", "mom2", "eps2")])


def _wgrad_workspace(x, cin, cout):
    return _scratch("conv wgrad", x.device, _lib.load().sc_conv3x3_wgrad_workspace_floats(cin, cout))


def basic_block_forward(x, pf1, pf2, g1, b1, g2, b2, bn1_state, bn2_state, split, groups):
    """out = relu(bn2(conv2(relu(bn1(conv1(x))))) + x) in one C call (sc_basic_block_forward): returns (out, saved) with saved =
    (y1, a1, y2, st1, st2) for basic_block_backward.  x must be what _aligned returns; the launches are those of conv3x3_apply /
    bn_act_forward, in their order."""
    B, C, H, _ = x.shape
    rm1, rv1, nt1, training, mom1, eps1 = bn1_state
    rm2, rv2, nt2, _, mom2, eps2 = bn2_state
    y1, a1, y2, out = (torch.empty_like(x) for _ in range(4))
    st = torch.empty(2, 2, groups, C, device=x.device, dtype=torch.float32)
    a = BlockArgs()
    a.x, a.pf1, a.pf2 = x.data_ptr(), pf1.data_ptr(), pf2.data_ptr()
    a.g1, a.b1, a.g2, a.b2 = g1.data_ptr(), b1.data_ptr(), g2.data_ptr(), b2.data_ptr()
    a.rm1, a.rv1, a.nt1, a.rm2, a.rv2, a.nt2 = _p(rm1), _p(rv1), _p(nt1), _p(rm2), _p(rv2), _p(nt2)
    a.y1, a.a1, a.y2, a.out = y1.data_ptr(), a1.data_ptr(), y2.data_ptr(), out.data_ptr()
    a.st1, a.st2 = st[0].data_ptr(), st[1].data_ptr()
    a.conv_ws, a.bn_ws = _conv_workspace(x.device, H, split).data_ptr(), _bn_partial(x, groups)
    a.batch, a.channels, a.hw, a.groups, a.training, a.split = B, C, H, groups, 1 if training else 0, 1 if split else 0
    a.mom1, a.eps1, a.mom2, a.eps2 = mom1, eps1, mom2, eps2
    code = _lib.load().sc_basic_block_forward(ctypes.byref(a), _lib.raw_stream(x.get_device()))
    if code:
        _lib.check(code, "sc_basic_block_forward")
    return out, (y1, a1, y2, st[0], st[1])


def basic_block_backward(d_out, x, saved, out, pb1, pb2, g1, b1, g2, b2, training, split, groups, need_dx, need_w1, need_w2):
    """Gradients of basic_block_forward in one C call (sc_basic_block_backward): (dx | None, gw1 | None, dgamma1, dbeta1, gw2 | None,
    dgamma2, dbeta2)."""
    y1, a1, y2, st1, st2 = saved
    B, C, H, _ = x.shape
    dy2, da1, dy1 = (torch.empty_like(x) for _ in range(3))
    dx, dres = (torch.empty_like(x), torch.empty_like(x)) if need_dx else (None, None)
    gw1 = torch.empty(C, C, 3, 3, device=x.device, dtype=torch.float32) if need_w1 else None
    gw2 = torch.empty(C, C, 3, 3, device=x.device, dtype=torch.float32) if need_w2 else None
    dgb = torch.empty(2, 2, C, device=x.device, dtype=torch.float32)
    a = BlockArgs()
    a.x, a.pb1, a.pb2, a.d_out = x.data_ptr(), pb1.data_ptr(), pb2.data_ptr(), d_out.data_ptr()
    a.g1, a.b1, a.g2, a.b2 = g1.data_ptr(), b1.data_ptr(), g2.data_ptr(), b2.data_ptr()
    a.y1, a.a1, a.y2, a.out, a.st1, a.st2 = y1.data_ptr(), a1.data_ptr(), y2.data_ptr(), out.data_ptr(), st1.data_ptr(), st2.data_ptr()
    a.dy2, a.da1, a.dy1, a.dres, a.dx = dy2.data_ptr(), da1.data_ptr(), dy1.data_ptr(), _p(dres), _p(dx)
    a.gw1, a.gw2, a.dgb1, a.dgb2 = _p(gw1), _p(gw2), dgb[0].data_ptr(), dgb[1].data_ptr()
    a.conv_ws, a.bn_ws = _conv_workspace(x.device, H, split).data_ptr(), _bn_partial(x, groups)
    a.wgrad_ws = _wgrad_workspace(x, C, C).data_ptr() if (need_w1 or need_w2) else None
    a.batch, a.channels, a.hw, a.groups, a.training, a.split, a.need_dx = B, C, H, groups, 1 if training else 0, 1 if split else 0, 1 if need_dx else 0
    code = _lib.load().sc_basic_block_backward(ctypes.byref(a), _lib.raw_stream(x.get_device()))
    if code:
        _lib.check(code, "sc_basic_block_backward")
    return dx, gw1, dgb[0, 0], dgb[0, 1], gw2, dgb[1, 0], dgb[1, 1]


def conv_stem_supported(x_shape, w_shape, stride=2, padding=3) -> bool:
    """Shapes sc_conv_stem_* take: [B, 3, 224, 224] inputs, a [64, 3, 7, 7] filter, stride 2, pad 3."""
    return (tuple(x_shape[1:]) == (3, 224, 224) and tuple(w_shape) == (64, 3, 7, 7) and stride in (2, (2, 2)) and padding in (3, (3, 3)))


def conv_stem_forward(x, w):
    lib = _lib.load()
    x, w = _aligned(x), _aligned(w)
    out = torch.empty(x.shape[0], 64, 112, 112, device=x.device, dtype=torch.float32)
    _lib.check(lib.sc_conv_stem_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(out), x.shape[0], _lib.stream()), "sc_conv_stem_forward")
    return out


def conv_stem_backward_weight(gy, x):
    lib = _lib.load()
    gy, x = _aligned(gy), _aligned(x)
    ws = _scratch("conv stem", x.device, lib.sc_conv_stem_wgrad_workspace_floats())
    dw = torch.empty(64, 3, 7, 7, device=x.device, dtype=torch.float32)
    _lib.check(lib.sc_conv_stem_wgrad(_lib.ptr(gy), _lib.ptr(x), _lib.ptr(dw), _lib.ptr(ws), x.shape[0], _lib.stream()), "sc_conv_stem_wgrad")
    return dw


def conv1x1s2_supported(x_shape, w_shape, stride=2, padding=0) -> bool:
    """Shapes sc_conv1x1s2_* take: a 1x1 filter, stride 2, no padding, square even maps, channel counts that are multiples of 64."""
    return (len(x_shape) == 4 and tuple(w_shape[2:]) == (1, 1) and stride in (2, (2, 2)) and padding in (0, (0, 0)) and x_shape[2] == x_shape[3]
            and x_shape[2] % 2 == 0 and w_shape[1] == x_shape[1] and w_shape[0] % 64 == 0 and w_shape[1] % 64 == 0)


def conv1x1s2_forward(x, w):
    lib = _lib.load()
    x, w = _aligned(x), _aligned(w)
    B, cin, H, _ = x.shape
    out = torch.empty(B, w.shape[0], H // 2, H // 2, device=x.device, dtype=torch.float32)
    _lib.check(lib.sc_conv1x1s2_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(out), B, cin, w.shape[0], H, _lib.stream()), "sc_conv1x1s2_forward")
    return out


def conv1x1s2_backward_data(gy, w):
    lib = _lib.load()
    gy, w = _aligned(gy), _aligned(w)
    B, cout, Ho, _ = gy.shape
    gx = torch.empty(B, w.shape[1], 2 * Ho, 2 * Ho, device=gy.device, dtype=torch.float32)
    _lib.check(lib.sc_conv1x1s2_backward_data(_lib.ptr(gy), _lib.ptr(w), _lib.ptr(gx), B, w.shape[1], cout, 2 * Ho, _lib.stream()),
               "sc_conv1x1s2_backward_data")
    return gx


def conv1x1s2_backward_weight(gy, x):
    lib = _lib.load()
    gy, x = _aligned(gy), _aligned(x)
    B, cin, H, _ = x.shape
    cout = gy.shape[1]
    n = lib.sc_conv1x1s2_wgrad_workspace_floats(cin, cout)
    ws = _scratch("conv 1x1s2", x.device, n)
    dw = torch.empty(cout, cin, 1, 1, device=x.device, dtype=torch.float32)
    _lib.check(lib.sc_conv1x1s2_wgrad(_lib.ptr(gy), _lib.ptr(x), _lib.ptr(dw), _lib.ptr(ws), B, cin, cout, H, _lib.stream()), "sc_conv1x1s2_wgrad")
    return dw


def conv3x3s2_supported(x_shape, w_shape, stride=2, padding=1) -> bool:
    """Shapes sc_conv3x3s2_forward takes: 3x3 filter, stride 2, pad 1, square 56 / 28 / 14 maps, channel counts that are multiples of 8."""
    return (len(x_shape) == 4 and tuple(w_shape[2:]) == (3, 3) and stride in (2, (2, 2)) and padding in (1, (1, 1)) and x_shape[2] == x_shape[3]
            and x_shape[2] in (56, 28, 14) and w_shape[1] == x_shape[1] and w_shape[0] % 8 == 0 and w_shape[1] % 8 == 0)


def conv3x3s2_forward(x, w):
    """F.conv2d(x, w, None, 2, 1) for x [B, Cin, H, H], w [Cout, Cin, 3, 3] (the stride-1 kernel with strided pixel offsets)."""
    lib = _lib.load()
    x, w = _aligned(x), _aligned(w)
    B, cin, H, _ = x.shape
    cout = w.shape[0]
    n = lib.sc_conv3x3s2_pack_floats(cin, cout, H)
    if n < 0:
        raise RuntimeError("shapeclipper_amd: sc_conv3x3s2 does not take [%d, %d, %d, %d] * %s" % (B, cin, H, H, tuple(w.shape)))
    w_pack = torch.empty(n, device=x.device, dtype=torch.float32)
    _lib.check(lib.sc_conv3x3_pack(_lib.ptr(w), _lib.ptr(w_pack), cin, cout, H, 4, _lib.stream()), "sc_conv3x3_pack")
    ws = _scratch("conv s2 %d" % H, x.device, lib.sc_conv3x3s2_workspace_floats(H))
    out = torch.empty(B, cout, H // 2, H // 2, device=x.device, dtype=torch.float32)
    _lib.check(lib.sc_conv3x3s2_forward(_lib.ptr(x), _lib.ptr(w_pack), _lib.ptr(out), _lib.ptr(ws), B, cin, cout, H, _lib.stream()),
               "sc_conv3x3s2_forward")
    return out


def conv3x3s2_grads_supported(x_shape, w_shape) -> bool:
    """Shapes sc_conv3x3s2_backward_data / sc_conv3x3s2_wgrad take: what conv3x3s2_supported takes, with channel counts that are multiples of 64."""
    return conv3x3s2_supported(x_shape, w_shape) and w_shape[0] % 64 == 0 and w_shape[1] % 64 == 0


def conv3x3s2_backward_data(gy, w, hw):
    """dL/dx [B, Cin, hw, hw] of F.conv2d(x, w, None, 2, 1) from gy [B, Cout, hw/2, hw/2] and the forward filter w [Cout, Cin, 3, 3]."""
    lib = _lib.load()
    gy, w = _aligned(gy), _aligned(w)
    B, cout = gy.shape[0], gy.shape[1]
    cin = w.shape[1]
    n = lib.sc_conv3x3s2_bd_pack_floats(cin, cout, hw)
    if n < 0 or tuple(gy.shape[2:]) != (hw // 2, hw // 2) or w.shape[0] != cout:
        raise RuntimeError("shapeclipper_amd: sc_conv3x3s2_backward_data does not take gy %s with w %s" % (tuple(gy.shape), tuple(w.shape)))
    w_pack = torch.empty(n, device=gy.device, dtype=torch.float32)
    _lib.check(lib.sc_conv3x3s2_bd_pack(_lib.ptr(w), _lib.ptr(w_pack), cin, cout, hw, _lib.stream()), "sc_conv3x3s2_bd_pack")
    ws = _scratch("conv s2bd %d" % hw, gy.device, lib.sc_conv3x3s2_bd_workspace_floats(hw))
    gx = torch.empty(B, cin, hw, hw, device=gy.device, dtype=torch.float32)
    _lib.check(lib.sc_conv3x3s2_backward_data(_lib.ptr(gy), _lib.ptr(w_pack), _lib.ptr(gx), _lib.ptr(ws), B, cin, cout, hw, _lib.stream()),
               "sc_conv3x3s2_backward_data")
    return gx


def conv3x3s2_backward_weight(gy, x):
    """dL/dw [Cout, Cin, 3, 3] of F.conv2d(x, w, None, 2, 1) from gy [B, Cout, hw/2, hw/2] and x [B, Cin, hw, hw]."""
    lib = _lib.load()
    gy, x = _aligned(gy), _aligned(x)
    B, cin, hw, _ = x.shape
    cout = gy.shape[1]
    n = lib.sc_conv3x3_wgrad_workspace_floats(cin, cout)
    if n < 0 or hw not in (56, 28, 14) or tuple(gy.shape) != (B, cout, hw // 2, hw // 2):
        raise RuntimeError("shapeclipper_amd: sc_conv3x3s2_wgrad does not take gy %s with x %s" % (tuple(gy.shape), tuple(x.shape)))
    ws = _scratch("conv wgrad", x.device, n)
    dw = torch.empty(cout, cin, 3, 3, device=x.device, dtype=torch.float32)
    _lib.check(lib.sc_conv3x3s2_wgrad(_lib.ptr(gy), _lib.ptr(x), _lib.ptr(dw), _lib.ptr(ws), B, cin, cout, hw, _lib.stream()), "sc_conv3x3s2_wgrad")
    return dw


class Conv3x3PackSet:
    """Kernel-ready filter images (forward and backward-data orientation) of MANY 3x3 / stride-1 convolutions, rewritten by ONE launch
    (sc_conv3x3_pack_multi): the filters of a network change once per optimizer step, so a trunk refreshes its set once per pass
    instead of packing twice per layer.  `items`: [(weight [Cout, Cin, 3, 3], map side)]."""

    def __init__(self, items, split=False):
        lib = _lib.load()
        self.split = bool(split)
        self.weights = [w for w, _ in items]
        self.ptrs = [w.data_ptr() for w in self.weights]
        rows, off, self.where = [], 0, {}
        for k, (w, side) in enumerate(items):
            if not (w.is_cuda and w.is_contiguous() and w.dtype == torch.float32):
                raise RuntimeError("shapeclipper_amd: Conv3x3PackSet needs contiguous fp32 device filters")
            for flip in (0, 1):
                cin, cout = (w.shape[0], w.shape[1]) if flip else (w.shape[1], w.shape[0])
                n = (lib.sc_conv3x3_pack_floats_split if split else lib.sc_conv3x3_pack_floats)(cin, cout, side)
                if n < 0:
                    raise RuntimeError("shapeclipper_amd: sc_conv3x3 does not take %dx%d maps with a %s filter" % (side, side, tuple(w.shape)))
                ct = (lib.sc_conv3x3_tile_channels_split if split else lib.sc_conv3x3_tile_channels)(side)
                rows.append([w.data_ptr(), off, cin, cout, ct, flip | (2 if split else 0)])
                self.where[(k, flip)] = (off, n)
                off += n
        if len(rows) > 128:
            raise RuntimeError("shapeclipper_amd: Conv3x3PackSet holds at most 64 filters (sc_conv3x3_pack_multi table limit)")
        dev = self.weights[0].device
        self.total = off
        # all rows split images with 64-channel tiles: the unit-per-workgroup pack kernel (coalesced reads, contiguous writes)
        self.units = bool(split) and all(r[4] == 64 for r in rows) and off % 13824 == 0
        self.table = torch.tensor(rows, dtype=torch.int64).to(dev)
        self.buf = torch.empty(off, device=dev, dtype=torch.float32)
        self.index = {id(w): k for k, w in enumerate(self.weights)}

    def stale(self):
        """True when a filter was re-allocated since the table was built (in-place optimizer updates keep the addresses)."""
        return any(w.data_ptr() != p for w, p in zip(self.weights, self.ptrs))

    def refresh(self):
        lib = _lib.load()
        fn = lib.sc_conv3x3_pack_multi_units if self.units else lib.sc_conv3x3_pack_multi
        _lib.check(fn(_lib.ptr(self.table), len(self.where), _lib.ptr(self.buf), self.total, _lib.stream()), "sc_conv3x3_pack_multi")

    def get(self, w, flip):
        off, n = self.where[(self.index[id(w)], int(flip))]
        return self.buf[off:off + n]


# ---- fused 1x1 bottleneck blocks (csrc/bottleneck.hip) ----------------------------------------------------------------------------------
def linear_bn_supported(N, Cin, Cout, groups) -> bool:
    return bool(_lib.load().sc_linear_bn_supported(N, Cin, Cout, groups))


def linear_bn_forward(x, w, gamma, beta, res, running_mean, running_var, n_tracked, training, momentum, eps, relu, groups):
    """out = [relu](bn(x w^T) [+ res]) in one launch -> (out, y, stats [2, G, Cout]).  x [N, Cin], w [Cout, Cin]."""
    N, Cin = x.shape
    Cout = w.shape[0]
    y, out = torch.empty(N, Cout, device=x.device, dtype=torch.float32), torch.empty(N, Cout, device=x.device, dtype=torch.float32)
    stats = torch.empty(2, groups, Cout, device=x.device, dtype=torch.float32)
    code = _lib.load().sc_linear_bn_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(res), _lib.ptr(y), _lib.ptr(out),
                                            _lib.ptr(stats[0]), _lib.ptr(stats[1]), _lib.ptr(running_mean), _lib.ptr(running_var), _lib.ptr(n_tracked),
                                            N, Cin, Cout, groups, 1 if training else 0, 1 if relu else 0,
                                            eps, momentum, _lib.stream())
    _lib.check(code, "sc_linear_bn_forward")
    return out, y, stats


def linear_bn_backward(g_out, gy_next, w_next, g_add, out, y, stats, gamma, x, want_res, training, relu, groups):
    """Reverse of linear_bn_forward -> (gy [N, Cout], g_res | None, dw [Cout, Cin], dgamma, dbeta).  The incoming gradient is g_out, or
    gy_next @ w_next when g_out is None, plus g_add."""
    N, Cin = x.shape
    Cout = y.shape[1]
    f32 = dict(device=x.device, dtype=torch.float32)
    gy = torch.empty(N, Cout, **f32)
    g_res = torch.empty(N, Cout, **f32) if want_res else None
    dw = torch.empty(Cout, Cin, **f32)
    dgb = torch.empty(2, Cout, **f32)
    code = _lib.load().sc_linear_bn_backward(_lib.ptr(g_out), _lib.ptr(gy_next), _lib.ptr(w_next), _lib.ptr(g_add),
                                             gy_next.shape[1] if gy_next is not None else 0, _lib.ptr(out), _lib.ptr(y), _lib.ptr(stats[0]),
                                             _lib.ptr(stats[1]), _lib.ptr(gamma), _lib.ptr(x), _lib.ptr(gy), _lib.ptr(g_res), _lib.ptr(dw),
                                             _lib.ptr(dgb[0]), _lib.ptr(dgb[1]), N, Cin, Cout, groups,
                                             1 if training else 0, 1 if relu else 0, _lib.stream())
    _lib.check(code, "sc_linear_bn_backward")
    return gy, g_res, dw, dgb[0], dgb[1]


def linear_backward_data(gy, w, g_add):
    """dx [N, Cin] = gy [N, Cout] @ w [Cout, Cin] (+ g_add)."""
    N, Cout = gy.shape
    Cin = w.shape[1]
    dx = torch.empty(N, Cin, device=gy.device, dtype=torch.float32)
    _lib.check(_lib.load().sc_linear_backward_data(_lib.ptr(gy), _lib.ptr(w), _lib.ptr(g_add), _lib.ptr(dx), N, Cin, Cout,
                                                   _lib.stream()), "sc_linear_backward_data")
    return dx


# ---- per-image latent biases (csrc/latent_bias.hip) --------------------------------------------------------------------------------------
def latent_bias_forward(z, lat, bias, post):
    B, Z = z.shape
    L, NL = lat.shape[0] // 64, bias.shape[0]
    out = torch.empty(B, NL, 64, device=z.device, dtype=torch.float32)
    _lib.check(_lib.load().sc_latent_bias_forward(_lib.ptr(z), _lib.ptr(lat), _lib.ptr(bias), _lib.ptr(post), _lib.ptr(out), B, Z, L,
                                                  NL, _lib.stream()), "sc_latent_bias_forward")
    return out


def latent_bias_backward(g, z, lat, post, NL, want_z=True):
    B, Z = z.shape
    L = lat.shape[0] // 64
    f32 = dict(device=z.device, dtype=torch.float32)
    g_z = torch.empty(B, Z, **f32) if want_z else None
    g_lat, g_bias = torch.empty(L * 64, Z, **f32), torch.empty(NL, 64, **f32)
    _lib.check(_lib.load().sc_latent_bias_backward(_lib.ptr(g), _lib.ptr(z), _lib.ptr(lat), _lib.ptr(post), _lib.ptr(g_z), _lib.ptr(g_lat), _lib.ptr(g_bias),
                                                   B, Z, L, NL, _lib.stream()), "sc_latent_bias_backward")
    return g_z, g_lat, g_bias


# ---- Pix3D loader: silhouette distance and weighted ray draw (csrc/silhouette_rays.hip) ----------------------------------
SILHOUETTE_MAX_SIDE = 512
_HIP_ERROR_INVALID_VALUE = 1


def _silhouette_shape(t, what):
    if t.dim() != 3:
        raise ValueError("shapeclipper_amd: %s takes [N,H,W], got shape %s" % (what, tuple(t.shape)))
    N, H, W = t.shape
    if not (1 <= H <= SILHOUETTE_MAX_SIDE and 1 <= W <= SILHOUETTE_MAX_SIDE):
        raise ValueError("shapeclipper_amd: %s supports 1 <= H, W <= %d, got %dx%d" % (what, SILHOUETTE_MAX_SIDE, H, W))
    return N, H, W


def silhouette_distance(masks: torch.Tensor) -> torch.Tensor:
    """masks [N,H,W] fp32 (inside: > 0.5) -> [N,H,W] fp32: distance from each pixel centre to the nearest pixel centre of the other
    class minus 0.5, bit-identical to float32(sqrt(float64(dx^2 + dy^2)) - 0.5); the image border is no boundary; a mask of one class
    only gives 0 everywhere (a uniform draw).  The boundary distance of the reference's compute_sampling_prob (utils/util.py:237-248)."""
    N, H, W = _silhouette_shape(masks, "silhouette_distance")
    masks = masks.contiguous().float()
    dist = torch.empty(N, H, W, device=masks.device, dtype=torch.float32)
    code = _lib.load().sc_silhouette_distance(_lib.ptr(masks), N, H, W, _lib.ptr(dist), _lib.stream())
    if code == _HIP_ERROR_INVALID_VALUE:
        raise ValueError("shapeclipper_amd: sc_silhouette_distance refused [%d,%d,%d]" % (N, H, W))
    _lib.check(code, "sc_silhouette_distance")
    return dist


def silhouette_rays(dist: torch.Tensor, n_rays: int, uniform_fac: float, seeds: torch.Tensor) -> torch.Tensor:
    """dist [N,H,W] fp32, seeds [N] int64 -> ray_idx [N,n_rays] int64: a draw of n_rays pixels without replacement with weights
    1 / (dist + uniform_fac), in the order of successive sampling (the law of np.random.choice(replace=False, p)).  Exponential race:
    the n_rays smallest keys -log(u_i) * (float64(dist_i) + uniform_fac), increasing, ties to the lower index; u_i in (0, 1] is a
    splitmix64 hash of (seed, i) (csrc/silhouette_rays.hip states it), so a mask's draw depends on its own seed only -- not on its
    place in the batch, N or the rank.  1 <= n_rays <= H*W; n_rays = H*W gives a permutation."""
    N, H, W = _silhouette_shape(dist, "silhouette_rays")
    n_rays = int(n_rays)
    if not 1 <= n_rays <= H * W:
        raise ValueError("shapeclipper_amd: silhouette_rays draws 1 <= n_rays <= H*W = %d rays without replacement, got %d" % (H * W, n_rays))
    if seeds.shape != (N,) or seeds.dtype != torch.int64:
        raise ValueError("shapeclipper_amd: silhouette_rays takes seeds [N] int64, got %s %s" % (tuple(seeds.shape), seeds.dtype))
    dist = dist.contiguous().float()
    seeds = seeds.to(dist.device).contiguous()
    ray_idx = torch.empty(N, n_rays, device=dist.device, dtype=torch.int64)
    code = _lib.load().sc_silhouette_rays(_lib.ptr(dist), N, H, W, n_rays, float(uniform_fac),
                                          _lib.ptr(seeds), _lib.ptr(ray_idx), _lib.stream())
    if code == _HIP_ERROR_INVALID_VALUE:
        raise ValueError("shapeclipper_amd: sc_silhouette_rays refused [%d,%d,%d], n_rays %d" % (N, H, W, n_rays))
    _lib.check(code, "sc_silhouette_rays")
    return ray_idx


# ---- CLIP annotation: the tower's input from Pix3D loader images (csrc/clip_preprocess.hip) ---------------------------------------
CLIP_PREPROCESS_MAX_SIDE = 16384
CLIP_PREPROCESS_MAX_NPX = 2048


def clip_preprocess(rgba: torch.Tensor, n_px: int, bgcolor, tables=None) -> torch.Tensor:
    """rgba [B,H,W,4] uint8 (the loader's resized RGBA images) -> [B,3,n_px,n_px] fp32, the CLIP tower's input: alpha >= 128 keeps the
    colour, else the background trunc(fp32(bgcolor) * 255) (bgcolor None: no composite); Pillow's bicubic resize of the short side
    to n_px; centre crop; (v / 255 - mean) / std.  Bit-identical to data/clip_preprocess.ClipPreprocess(n_px, bgcolor) on each image.
    `tables`: the int32 device tensors of clip_preprocess.kernel_tables(H, W, n_px) (built here when None)."""
    from .data import clip_preprocess as cp
    if rgba.dim() != 4 or rgba.shape[3] != 4 or rgba.dtype != torch.uint8:
        raise ValueError("shapeclipper_amd: clip_preprocess takes [B,H,W,4] uint8, got %s %s" % (tuple(rgba.shape), rgba.dtype))
    B, H, W, _ = rgba.shape
    n_px = int(n_px)
    if not (1 <= H <= CLIP_PREPROCESS_MAX_SIDE and 1 <= W <= CLIP_PREPROCESS_MAX_SIDE and 1 <= n_px <= CLIP_PREPROCESS_MAX_NPX):
        raise ValueError("shapeclipper_amd: clip_preprocess supports 1 <= H, W <= %d and 1 <= n_px <= %d, got %dx%d -> %d"
                         % (CLIP_PREPROCESS_MAX_SIDE, CLIP_PREPROCESS_MAX_SIDE, H, W, n_px))
    if bgcolor is not None and not 0.0 <= float(bgcolor) <= 1.0:
        raise ValueError("shapeclipper_amd: clip_preprocess takes bgcolor None or in [0, 1], got %r" % (bgcolor,))
    if tables is None:
        tables = tuple(torch.from_numpy(a).to(rgba.device) for a in cp.kernel_tables(H, W, n_px))
    hb, hk, vb, vk = tables
    if not (hb.shape == (n_px, 2) and vb.shape == (n_px, 2) and hk.dim() == 2 and hk.shape[0] == n_px and vk.dim() == 2
            and vk.shape[0] == n_px and all(t.dtype == torch.int32 for t in tables)):
        raise ValueError("shapeclipper_amd: clip_preprocess tables do not match n_px %d" % n_px)
    rgba = rgba.contiguous()
    out = torch.empty(B, 3, n_px, n_px, device=rgba.device, dtype=torch.float32)
    if B == 0:
        return out
    tmp = torch.empty(B, H, n_px, 4, device=rgba.device, dtype=torch.uint8)
    code = _lib.load().sc_clip_preprocess(_lib.ptr(rgba), B, H, W, n_px, cp.background_byte(bgcolor),
                                          _lib.ptr(hb.contiguous()), _lib.ptr(hk.contiguous()), hk.shape[1],
                                          _lib.ptr(vb.contiguous()), _lib.ptr(vk.contiguous()), vk.shape[1],
                                          _lib.ptr(tmp), _lib.ptr(out), _lib.stream())
    if code == _HIP_ERROR_INVALID_VALUE:
        raise ValueError("shapeclipper_amd: sc_clip_preprocess refused [%d,%d,%d,4] -> %d" % (B, H, W, n_px))
    _lib.check(code, "sc_clip_preprocess")
    return out


# ---- training-time visualisation: turn-table GIF frames (csrc/vis_frames.hip) -----------------------------------------------------
VIS_FRAME_KINDS = dict(rgb=(0, 3), mask=(1, 1), normal=(2, 3))      # kind -> (code, channels per pixel)


def vis_frames(x: torch.Tensor, kind: str, from_range=(0, 1)) -> torch.Tensor:
    """x [..., c] fp32 per-ray outputs of the render chain (c = 3 for "rgb" and "normal", 1 for "mask"; an image's rays in row-major pixel
    order) -> uint8 [..., 3], the frame bytes the reference's dump_gifs hands to PIL: "rgb" trunc(clamp((x - lo) / (hi - lo), 0, 1) * 255);
    "normal" the same of x / 2 + 0.5 (vis_rotate's normal maps); "mask" matplotlib's `gray` colormap as get_heatmap applies it, index
    trunc(v * 256) with 256 -> 255 on all three channels.  NaN gives 0.  One launch."""
    import numpy as np
    if kind not in VIS_FRAME_KINDS:
        raise ValueError("shapeclipper_amd: vis_frames kind is one of %s, got %r" % (sorted(VIS_FRAME_KINDS), kind))
    code, c = VIS_FRAME_KINDS[kind]
    if x.dtype != torch.float32 or x.dim() < 1 or x.shape[-1] != c:
        raise ValueError("shapeclipper_amd: vis_frames(%s) takes [..., %d] fp32, got %s %s" % (kind, c, tuple(x.shape), x.dtype))
    lo, hi = from_range
    scale = float(np.float32(1.0) / np.float32(hi - lo))        # torch divides by a Python number as a multiply by its fp32 reciprocal
    x = x.contiguous()
    out = torch.empty(*x.shape[:-1], 3, device=x.device, dtype=torch.uint8)
    code = _lib.load().sc_vis_frames(_lib.ptr(x), x.numel() // c, c, code, lo,
                                     scale, _lib.ptr(out), _lib.stream())
    _lib.check(code, "sc_vis_frames")
    return out


# ---- Chamfer3D backward in a fixed summation order (csrc/chamfer_bwd.hip) -----------------------------------------------------------
def chamfer_backward_ordered(xyz1, xyz2, graddist1, graddist2, idx1, idx2, want1=True, want2=True):
    """-> (gradxyz1 [b,n,3] or None, gradxyz2 [b,m,3] or None): sc_chamfer3d_backward_ordered on torch's current stream; the gradient
    that is not wanted is not formed.  Inputs fp32 / int32, contiguous, on one device (the caller checks); the workspace is the
    "chamfer bwd" buffer of the scratch cache."""
    lib = _lib.load()
    b, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    g1 = torch.empty_like(xyz1) if want1 else None
    g2 = torch.empty_like(xyz2) if want2 else None
    words = (lib.sc_chamfer3d_backward_ordered_workspace_bytes(b, n, m) + 3) // 4
    ws = _scratch("chamfer bwd", xyz1.device, words) if words else None
    code = lib.sc_chamfer3d_backward_ordered(_lib.ptr(xyz1), _lib.ptr(xyz2), _lib.ptr(g1), _lib.ptr(g2), _lib.ptr(graddist1),
                                             _lib.ptr(graddist2), _lib.ptr(idx1), _lib.ptr(idx2), b, n, m, _lib.ptr(ws), _lib.stream())
    _lib.check(code, "sc_chamfer3d_backward_ordered")
    return g1, g2


# ---- evaluation: similarity ICP of the prediction onto the ground truth (csrc/icp.hip; the search is chamfer_3D's) -----------------
ICP_MAX_ITERS = 100
ICP_MAX_IMAGES = 65535
IcpResult = collections.namedtuple("IcpResult", ["transform", "s", "aligned", "dist1", "dist2", "idx1", "idx2", "objective"])


def _icp_check(who, dev, **tensors):
    """chamfer_3D._check for the ICP entry points (raw pointers go to the C ABI): TypeError for a wrong dtype, ValueError for a wrong
    shape, another device or a non-contiguous tensor, RuntimeError for host tensors."""
    if dev.type != "cuda":
        raise RuntimeError(_lib.NO_CPU)
    for name, (t, dtype, shape) in tensors.items():
        if not isinstance(t, torch.Tensor):
            raise TypeError("shapeclipper_amd: %s: %s must be a tensor, got %s" % (who, name, type(t).__name__))
        if t.dtype != dtype:
            raise TypeError("shapeclipper_amd: %s: %s must be %s, got %s" % (who, name, dtype, t.dtype))
        if tuple(t.shape) != tuple(shape):
            raise ValueError("shapeclipper_amd: %s: %s must have shape %s, got %s" % (who, name, tuple(shape), tuple(t.shape)))
        if t.device != dev:
            raise ValueError("shapeclipper_amd: %s: %s is on %s, src is on %s" % (who, name, t.device, dev))
        if not t.is_contiguous():
            raise ValueError("shapeclipper_amd: %s: %s must be contiguous" % (who, name))


def _icp_dims(who, src, dst=None):
    """(B, N[, M]) of src [B,N,3] (and dst [B,M,3]); ValueError for another rank, a mismatched B, an empty cloud or B > 65535."""
    for name, t in (("src", src), ("dst", dst)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[2] != 3 or t.shape[1] < 1):
            raise ValueError("shapeclipper_amd: %s: %s must be [B,N,3] with N >= 1, got %s" % (
                who, name, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))
    if src.shape[0] > ICP_MAX_IMAGES:
        raise ValueError("shapeclipper_amd: %s takes at most %d images per call, got %d" % (who, ICP_MAX_IMAGES, src.shape[0]))
    if dst is None:
        return src.shape[0], src.shape[1]
    if dst.shape[0] != src.shape[0]:
        raise ValueError("shapeclipper_amd: %s: src has %d images, dst has %d" % (who, src.shape[0], dst.shape[0]))
    return src.shape[0], src.shape[1], dst.shape[1]


def _icp_workspace(lib, dev, B, N, M):
    return _scratch("icp", dev, (lib.sc_icp_workspace_bytes(B, N, M) + 3) // 4) if B else None


def icp_fit(src, dst, idx1, idx2, scale=True):
    """src [B,N,3], dst [B,M,3] fp32, idx1 [B,N], idx2 [B,M] int32 (the nearest-neighbour indices chamfer_3D.forward writes for the
    CURRENT source points against dst) -> (transform [B,4,4] float64, s [B] float64): the similarity (or rigid, scale=False) transform
    that minimises the summed squared distance of the pairs (src[i], dst[idx1[i]]) / N and (src[idx2[j]], dst[j]) / M, by Umeyama's
    closed form in float64 (sc_icp_fit; include/shapeclipper_hip.h states every sum's order).  transform = [s R, t; 0 0 0 1].  An image
    whose sums are not finite or whose source pairs have rank <= 1 (one point, collinear points) gets the identity and s = 1."""
    B, N, M = _icp_dims("icp_fit", src, dst)
    i32 = torch.int32
    _icp_check("icp_fit", src.device, src=(src, torch.float32, (B, N, 3)), dst=(dst, torch.float32, (B, M, 3)),
               idx1=(idx1, i32, (B, N)), idx2=(idx2, i32, (B, M)))
    lib = _lib.load()
    T = torch.empty(B, 4, 4, device=src.device, dtype=torch.float64)
    s = torch.empty(B, device=src.device, dtype=torch.float64)
    with torch.cuda.device(src.device):
        ws = _icp_workspace(lib, src.device, B, N, M)
        code = lib.sc_icp_fit(_lib.ptr(src), _lib.ptr(dst), _lib.ptr(idx1), _lib.ptr(idx2), B, N, M, int(bool(scale)), None, None,
                              _lib.ptr(ws), _lib.ptr(T), _lib.ptr(s), _lib.stream())
    _lib.check(code, "sc_icp_fit")
    return T, s


def icp_apply(src, transform):
    """src [B,N,3] fp32, transform [B,4,4] float64 -> [B,N,3] fp32: fp32(((m00 x + m01 y) + m02 z) + t0) per coordinate, formed in float64
    without contraction and rounded once (sc_icp_apply); the last row of transform is not read."""
    B, N = _icp_dims("icp_apply", src)
    _icp_check("icp_apply", src.device, src=(src, torch.float32, (B, N, 3)), transform=(transform, torch.float64, (B, 4, 4)))
    lib = _lib.load()
    out = torch.empty_like(src)
    with torch.cuda.device(src.device):
        code = lib.sc_icp_apply(_lib.ptr(src), _lib.ptr(transform), B, N, _lib.ptr(out), _lib.stream())
    _lib.check(code, "sc_icp_apply")
    return out


def icp_objective(dist1, dist2):
    """dist1 [B,N], dist2 [B,M] fp32 (chamfer_3D.forward's squared distances) -> [B] float64 mean(dist1) + mean(dist2), summed in float64
    in sc_icp_objective's fixed order: the quantity icp_align records per iteration."""
    if not isinstance(dist1, torch.Tensor) or not isinstance(dist2, torch.Tensor) or dist1.dim() != 2 or dist2.dim() != 2 \
            or dist1.shape[0] != dist2.shape[0] or dist1.shape[1] < 1 or dist2.shape[1] < 1 or dist1.shape[0] > ICP_MAX_IMAGES:
        raise ValueError("shapeclipper_amd: icp_objective takes dist1 [B,N] and dist2 [B,M] with B <= %d" % ICP_MAX_IMAGES)
    B, N, M = dist1.shape[0], dist1.shape[1], dist2.shape[1]
    _icp_check("icp_objective", dist1.device, dist1=(dist1, torch.float32, (B, N)), dist2=(dist2, torch.float32, (B, M)))
    lib = _lib.load()
    out = torch.empty(B, device=dist1.device, dtype=torch.float64)
    with torch.cuda.device(dist1.device):
        ws = _icp_workspace(lib, dist1.device, B, N, M)
        code = lib.sc_icp_objective(_lib.ptr(dist1), _lib.ptr(dist2), B, N, M, _lib.ptr(ws), _lib.ptr(out), 1, _lib.stream())
    _lib.check(code, "sc_icp_objective")
    return out


def icp_align(src, dst, iters=30, scale=True):
    """src [B,N,3], dst [B,M,3] fp32 -> IcpResult: `iters` rounds of (apply the transform to src, search both directions, fit), then one
    last apply and search.  The count is fixed -- no convergence test, so no host synchronisation, and the result is reproducible bit
    for bit.  The search is chamfer_3D.forward's (its path selection and chamfer_3D.SEARCH hold, ties as there), its workspace and outputs
    allocated once.  Every fit pairs the ORIGINAL source points with dst, so the transform is absolute and nothing accumulates over the
    rounds; a round whose fit is degenerate (icp_fit) keeps the transform it had.

    transform [B,4,4] float64 = [s R, t; 0 0 0 1] and s [B] float64 after the last fit; aligned [B,N,3] = icp_apply(src, transform);
    dist1 [B,N], dist2 [B,M] (squared, as Chamfer returns them), idx1, idx2 of the last search (aligned against dst); objective
    [B, iters+1] float64, objective[:, j] = mean(dist1) + mean(dist2) under the transform after j fits (column 0: the input's own).
    ValueError for iters outside 1..100; icp_fit's checks otherwise."""
    if isinstance(iters, bool) or not isinstance(iters, int) or not 1 <= iters <= ICP_MAX_ITERS:
        raise ValueError("shapeclipper_amd: icp_align needs an integer iters in 1..%d, got %r" % (ICP_MAX_ITERS, iters))
    B, N, M = _icp_dims("icp_align", src, dst)
    _icp_check("icp_align", src.device, src=(src, torch.float32, (B, N, 3)), dst=(dst, torch.float32, (B, M, 3)))
    import chamfer_3D
    lib = _lib.load()
    dev = src.device
    f32, f64, i32 = torch.float32, torch.float64, torch.int32
    T = torch.eye(4, device=dev, dtype=f64).repeat(B, 1, 1)
    s = torch.ones(B, device=dev, dtype=f64)
    cur = torch.empty_like(src)
    d1, d2 = torch.empty(B, N, device=dev, dtype=f32), torch.empty(B, M, device=dev, dtype=f32)
    i1, i2 = torch.empty(B, N, device=dev, dtype=i32), torch.empty(B, M, device=dev, dtype=i32)
    objective = torch.empty(B, iters + 1, device=dev, dtype=f64)
    if B == 0:
        return IcpResult(T, s, cur, d1, d2, i1, i2, objective)
    with torch.cuda.device(dev):
        search_ws = chamfer_3D._workspace(lib, B, N, M, dev)
        ws = _icp_workspace(lib, dev, B, N, M)
        p = _lib.ptr
        for j in range(iters + 1):
            _lib.check(lib.sc_icp_apply(p(src), p(T), B, N, p(cur), _lib.stream()), "sc_icp_apply")
            chamfer_3D._forward(lib, B, N, M, cur, dst, d1, d2, i1, i2, ws=search_ws)
            col = ctypes.c_void_p(objective.data_ptr() + 8 * j)
            _lib.check(lib.sc_icp_objective(p(d1), p(d2), B, N, M, p(ws), col, iters + 1, _lib.stream()), "sc_icp_objective")
            if j < iters:
                _lib.check(lib.sc_icp_fit(p(src), p(dst), p(i1), p(i2), B, N, M, int(bool(scale)), p(T), p(s), p(ws), p(T), p(s),
                                          _lib.stream()), "sc_icp_fit")
    return IcpResult(T, s, cur, d1, d2, i1, i2, objective)


# ---- evaluation: k nearest neighbours, PCA normals and normal consistency (csrc/point_normals.hip) -----------------------------------
KNN_MIN_K, KNN_MAX_K = 3, 32
PointNormals = collections.namedtuple("PointNormals", ["normals", "variation", "idx", "dist"])


def _knn_args(who, points, k):
    """(B, N) of points [B,N,3] fp32 for a k in 3..32 with N >= k: _icp_dims' and _icp_check's refusals, ValueError for the k."""
    if isinstance(k, bool) or not isinstance(k, int) or not KNN_MIN_K <= k <= KNN_MAX_K:
        raise ValueError("shapeclipper_amd: %s needs an integer k in %d..%d, got %r" % (who, KNN_MIN_K, KNN_MAX_K, k))
    B, N = _icp_dims(who, points)
    _icp_check(who, points.device, points=(points, torch.float32, (B, N, 3)))
    if N < k:
        raise ValueError("shapeclipper_amd: %s: %d points per image are fewer than k = %d" % (who, N, k))
    return B, N


def knn_points(points, k):
    """points [B,N,3] fp32 -> (idx [B,N,k] int32, dist [B,N,k] fp32): for every point the k nearest points of its own image, itself
    included, by the key (bits of d, index) ascending with d = (dx dx + dy dy) + dz dz in fp32 -- an exact grid search (sc_knn_points;
    include/shapeclipper_hip.h states the order and the search).  ValueError for k outside 3..32 or N < k."""
    B, N = _knn_args("knn_points", points, k)
    lib = _lib.load()
    idx = torch.empty(B, N, k, device=points.device, dtype=torch.int32)
    dist = torch.empty(B, N, k, device=points.device, dtype=torch.float32)
    if B == 0:
        return idx, dist
    with torch.cuda.device(points.device):
        ws = _scratch("knn", points.device, (lib.sc_knn_workspace_bytes(B, N, k) + 3) // 4)
        code = lib.sc_knn_points(_lib.ptr(points), B, N, k, _lib.ptr(ws), _lib.ptr(idx), _lib.ptr(dist), _lib.stream())
    _lib.check(code, "sc_knn_points")
    return idx, dist


def point_normals(points, k=16, idx=None):
    """points [B,N,3] fp32 -> PointNormals(normals [B,N,3] fp32, variation [B,N] fp32, idx [B,N,k] int32, dist [B,N,k] fp32 or None): the
    PCA normal of every point's k nearest neighbours (knn_points, or the idx [B,N,k] handed in, whose dist is then None) -- the
    eigenvector of the smallest eigenvalue of their float64 covariance, unit, UNORIENTED (its largest component is made positive) -- and
    the surface variation l0 / (l0 + l1 + l2).  Collinear, coincident or non-finite neighbourhoods get normal 0 and variation 0
    (sc_point_normals)."""
    B, N = _knn_args("point_normals", points, k)
    dist = None
    if idx is None:
        idx, dist = knn_points(points, k)
    else:
        _icp_check("point_normals", points.device, idx=(idx, torch.int32, (B, N, k)))
    lib = _lib.load()
    normals = torch.empty(B, N, 3, device=points.device, dtype=torch.float32)
    variation = torch.empty(B, N, device=points.device, dtype=torch.float32)
    with torch.cuda.device(points.device):
        code = lib.sc_point_normals(_lib.ptr(points), _lib.ptr(idx), B, N, k, _lib.ptr(normals), _lib.ptr(variation), _lib.stream())
    _lib.check(code, "sc_point_normals")
    return PointNormals(normals, variation, idx, dist)


def normal_consistency(n1, n2, idx1, idx2):
    """n1 [B,N,3], n2 [B,M,3] fp32 normals of two clouds, idx1 [B,N], idx2 [B,M] int32 (chamfer_3D.forward's nearest neighbours of the
    clouds) -> (acc [B], comp [B]) float64: mean_i |n1[i] . n2[idx1[i]]| and mean_j |n2[j] . n1[idx2[j]]|, summed in float64 in
    sc_icp_objective's fixed order (sc_normal_consistency).  An index outside its cloud makes that image's value NaN."""
    B, N, M = _icp_dims("normal_consistency", n1, n2)
    i32 = torch.int32
    _icp_check("normal_consistency", n1.device, n1=(n1, torch.float32, (B, N, 3)), n2=(n2, torch.float32, (B, M, 3)),
               idx1=(idx1, i32, (B, N)), idx2=(idx2, i32, (B, M)))
    lib = _lib.load()
    acc = torch.empty(B, device=n1.device, dtype=torch.float64)
    comp = torch.empty(B, device=n1.device, dtype=torch.float64)
    with torch.cuda.device(n1.device):
        ws = _icp_workspace(lib, n1.device, B, N, M)
        code = lib.sc_normal_consistency(_lib.ptr(n1), _lib.ptr(n2), _lib.ptr(idx1), _lib.ptr(idx2), B, N, M, _lib.ptr(ws), _lib.ptr(acc),
                                         _lib.ptr(comp), _lib.stream())
    _lib.check(code, "sc_normal_consistency")
    return acc, comp


# ---- evaluation: exact distance from points to a triangle mesh (csrc/point_mesh.hip) --------------------------------------------------
POINT_MESH_MAX_IMAGES = 65535
POINT_MESH_MAX_FACES = 1 << 26
PointMesh = collections.namedtuple("PointMesh", ["dist2", "face", "closest"])


def _point_mesh_args(points, verts, faces, v_count, f_count, search):
    """(B, N, Vtot, Ftot) of point_mesh_distance's arguments; every refusal is a ValueError (the index check is the caller's)."""
    who = "shapeclipper_amd: point_mesh_distance"
    if search not in ("grid", "brute"):
        raise ValueError("%s: search must be 'grid' or 'brute', got %r" % (who, search))
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    for name, t, dtypes in (("points", points, (f32,)), ("verts", verts, (f32,)), ("faces", faces, (i32,)), ("v_count", v_count, (i32, i64)),
                            ("f_count", f_count, (i32, i64))):
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s: %s must be a tensor, got %s" % (who, name, type(t).__name__))
        if not t.is_cuda and not name.endswith("_count"):               # the counts may be on the host, where the producers leave them
            raise ValueError("%s: %s is a CPU tensor; the HIP kernels need device tensors (no CPU fallback)" % (who, name))
        if t.is_cuda and t.device != points.device:
            raise ValueError("%s: %s is on %s, points is on %s" % (who, name, t.device, points.device))
        if t.dtype not in dtypes:
            raise ValueError("%s: %s must be %s, got %s" % (who, name, " or ".join(str(d) for d in dtypes), t.dtype))
        if not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous" % (who, name))
    if v_count.dtype != f_count.dtype or v_count.device != f_count.device:
        raise ValueError("%s: v_count and f_count must come in one form, got %s on %s and %s on %s"
                         % (who, v_count.dtype, v_count.device, f_count.dtype, f_count.device))
    if points.dim() != 3 or points.shape[2] != 3 or points.shape[1] < 1:
        raise ValueError("%s: points must be [B,N,3] with N >= 1, got %s" % (who, tuple(points.shape)))
    B, N = points.shape[0], points.shape[1]
    for name, t in (("verts", verts), ("faces", faces)):
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError("%s: %s must be [n,3], got %s" % (who, name, tuple(t.shape)))
    for name, t in (("v_count", v_count), ("f_count", f_count)):
        if tuple(t.shape) != (B,):
            raise ValueError("%s: %s must have shape (%d,), got %s" % (who, name, B, tuple(t.shape)))
    if B > POINT_MESH_MAX_IMAGES or B * N > 1 << 30 or faces.shape[0] > POINT_MESH_MAX_FACES:
        raise ValueError("%s takes at most %d images, 2^30 queries and 2^26 faces per call, got %d, %d and %d"
                         % (who, POINT_MESH_MAX_IMAGES, B, B * N, faces.shape[0]))
    return B, N, verts.shape[0], faces.shape[0]


def point_mesh_distance(points, verts, faces, v_count, f_count, search="grid"):
    """points [B,N,3] fp32 against the PackedMesh (mesh_pack.py) of B images, passed as `*mesh` -- verts [Vtot,3] fp32 and faces [Ftot,3]
    int32 on points' device; v_count / f_count [B], both in one form: int64 or int32, on the host (as every producer returns them) or on
    that device.  The C entry point takes int32 device counts; that form is passed through, any other is converted (two copies, no read)
    -> PointMesh(dist2 [B,N] fp32, face [B,N] int32, closest [B,N,3] fp32): for every point the squared distance to the nearest
    triangle of its image, that triangle's local index (the LOWEST among exact ties) and the closest point on it, in the fp32 arithmetic
    include/shapeclipper_hip.h states for sc_point_mesh_distance (PyTorch3D's point_mesh_face_distance keeps the distance only).
    search="grid": the exact uniform-grid search; search="brute": all pairs, the same bits.  An image without faces gets +Inf, -1, 0; a
    point that is not finite NaN, -1, NaN.

    Host synchronisation: ONE device reduction and host read per call, which validates the inputs -- the counts must be non-negative and
    sum to the packed lengths, every face index must lie inside its image's vertex range (ValueError otherwise).  The search itself
    reads nothing back: its workspace has a fixed capacity (the `_scratch` cache, tag "point_mesh"; faces that overlap more than 16
    cells go on a per-image list instead of the grid).  Runs on the current stream."""
    B, N, Vtot, Ftot = _point_mesh_args(points, verts, faces, v_count, f_count, search)
    dev = points.device
    dist2 = torch.empty(B, N, device=dev, dtype=torch.float32)
    face = torch.empty(B, N, device=dev, dtype=torch.int32)
    closest = torch.empty(B, N, 3, device=dev, dtype=torch.float32)
    if B == 0:
        return PointMesh(dist2, face, closest)
    # the one reduction: (counts non-negative, sum of v_count, sum of f_count, faces inside their image's vertex range) -> 4 numbers
    vc, fc = v_count.to(dev).long(), f_count.to(dev).long()
    if not v_count.is_cuda or v_count.dtype != torch.int32:
        v_count, f_count = vc.int(), fc.int()                           # the validated int64 values below bound them
    inside = torch.ones((), dtype=torch.bool, device=dev)
    if Ftot:        # the image of every packed face, from the running sum of f_count (no host read; meaningful only if the sums hold)
        owner = torch.searchsorted(torch.cumsum(fc.clamp_min(0), 0), torch.arange(Ftot, device=dev), right=True).clamp_max(B - 1)
        inside = ((faces >= 0) & (faces < vc[owner][:, None])).all()
    ok_counts, v_sum, f_sum, ok_faces = torch.stack([((vc >= 0) & (fc >= 0)).all().long(), vc.sum(), fc.sum(), inside.long()]).tolist()
    if not ok_counts or v_sum != Vtot or f_sum != Ftot:
        raise ValueError("shapeclipper_amd: point_mesh_distance: v_count / f_count must be non-negative and sum to the packed lengths "
                         "(%d vertices, %d faces), got sums %d and %d" % (Vtot, Ftot, v_sum, f_sum))
    if not ok_faces:
        raise ValueError("shapeclipper_amd: point_mesh_distance: a face index lies outside its image's vertex range [0, v_count[b])")
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = _scratch("point_mesh", dev, (lib.sc_point_mesh_workspace_bytes(B, N, Vtot, Ftot) + 3) // 4)
        fn = lib.sc_point_mesh_distance if search == "grid" else lib.sc_point_mesh_distance_brute
        code = fn(_lib.ptr(points), _lib.ptr(verts) if Vtot else None, _lib.ptr(faces) if Ftot else None, _lib.ptr(v_count),
                  _lib.ptr(f_count), B, N, Vtot, Ftot, _lib.ptr(ws), _lib.ptr(dist2), _lib.ptr(face), _lib.ptr(closest), _lib.stream())
    _lib.check(code, "sc_point_mesh_distance" if search == "grid" else "sc_point_mesh_distance_brute")
    return PointMesh(dist2, face, closest)


# ---- evaluation: Earth Mover's Distance by an auction matching (csrc/emd3d.hip) --------------------------------------------------------
EMD_MAX_POINTS = 2048           # SC_EMD3D_MAX_POINTS
EMD_MAX_PHASES = 80             # SC_EMD3D_MAX_PHASES
EMD_MAX_IMAGES = 65535
EmdResult = collections.namedtuple("EmdResult", ["assignment", "cost", "price", "emd", "rounds", "converged"])


def emd_eps_list(eps=1e-4, eps_start=0.25):
    """The epsilon of every phase of the auction as fp32 values (Python floats that hold them exactly): e = eps_start; while e > eps:
    emit e, e = fl(e / 4); then emit eps -- include/shapeclipper_hip.h, sc_emd3d_match.  0.25 and 1e-4 give 7 phases."""
    f32 = lambda x: ctypes.c_float(x).value         # one rounding to fp32
    eps, e, out = f32(eps), f32(eps_start), []
    while e > eps:
        out.append(e)
        e = f32(e / 4.0)                            # the float64 quotient of an fp32 value by 4 is exact; rounded once
    out.append(eps)
    return out


def _emd_args(xyz1, xyz2, eps, eps_start, max_rounds):
    """(B, n, eps list) of emd_match's arguments.  TypeError for something that is not an fp32 tensor, ValueError for shapes, sizes and
    settings -- all before the device is looked at -- then RuntimeError for host tensors (as the ICP entry points) and ValueError for
    another device or a non-contiguous tensor."""
    who = "shapeclipper_amd: emd_match"
    for name, t in (("xyz1", xyz1), ("xyz2", xyz2)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a tensor, got %s" % (who, name, type(t).__name__))
        if t.dtype != torch.float32:
            raise TypeError("%s: %s must be torch.float32, got %s" % (who, name, t.dtype))
    if xyz1.dim() != 3 or xyz1.shape[2] != 3 or tuple(xyz2.shape) != tuple(xyz1.shape):
        raise ValueError("%s: xyz1 and xyz2 must have one shape [B,n,3], got %s and %s" % (who, tuple(xyz1.shape), tuple(xyz2.shape)))
    B, n = xyz1.shape[0], xyz1.shape[1]
    if not 2 <= n <= EMD_MAX_POINTS:
        raise ValueError("%s: n must be in 2..%d, got %d" % (who, EMD_MAX_POINTS, n))
    if B > EMD_MAX_IMAGES:
        raise ValueError("%s takes at most %d images per call, got %d" % (who, EMD_MAX_IMAGES, B))
    for name, v in (("eps", eps), ("eps_start", eps_start)):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise TypeError("%s: %s must be a real number, got %r" % (who, name, v))
    if not 0.0 < eps <= eps_start or not ctypes.c_float(eps_start).value < float("inf") or not ctypes.c_float(eps).value > 0.0:
        raise ValueError("%s: need 0 < eps <= eps_start (both fp32 numbers: eps_start finite, eps not below the smallest), got eps = %r, eps_start = %r"
                         % (who, eps, eps_start))
    if isinstance(max_rounds, bool) or not isinstance(max_rounds, int):
        raise TypeError("%s: max_rounds must be an integer, got %r" % (who, max_rounds))
    if not 1 <= max_rounds < 1 << 31:
        raise ValueError("%s: max_rounds must be in 1..2^31 - 1, got %r" % (who, max_rounds))
    phases = emd_eps_list(eps, eps_start)
    if len(phases) > EMD_MAX_PHASES:
        raise ValueError("%s: eps = %r, eps_start = %r need %d phases, at most %d" % (who, eps, eps_start, len(phases), EMD_MAX_PHASES))
    if not xyz1.is_cuda or not xyz2.is_cuda:
        raise RuntimeError(_lib.NO_CPU)
    if xyz2.device != xyz1.device:
        raise ValueError("%s: xyz2 is on %s, xyz1 is on %s" % (who, xyz2.device, xyz1.device))
    if not xyz1.is_contiguous() or not xyz2.is_contiguous():
        raise ValueError("%s: xyz1 and xyz2 must be contiguous" % who)
    return B, n, phases


def emd_match(xyz1, xyz2, eps=1e-4, eps_start=0.25, max_rounds=1 << 18):
    """xyz1, xyz2 [B,n,3] fp32, 2 <= n <= 2048 -> EmdResult(assignment [B,n] int32, cost [B,n] fp32, price [B,n] fp32, emd [B] float64,
    rounds [B] int32, converged [B] int32): per image the one-to-one matching of the points of xyz1 (persons) to those of xyz2 (objects)
    that minimises the summed Euclidean distance of the pairs to within n eps, by a forward auction with epsilon scaling from eps_start
    down to eps (include/shapeclipper_hip.h, sc_emd3d_match, states the rule; csrc/emd3d.hip runs one workgroup per image).
    assignment[b, i] is the object of person i, cost its distance, price the objects' final prices, emd the float64 mean of cost --
    the Earth Mover's Distance of the two clouds, at most eps above the optimum when converged is 1.  After max_rounds rounds the
    auction stops, completes the matching in index order and reports converged 0.  An image with a non-finite coordinate gets the
    identity, zeros, converged 0 and emd NaN.  No gradient.  The same bits from run to run, alone or in a batch.

    Host synchronisation: none.  Runs on the current stream."""
    B, n, phases = _emd_args(xyz1, xyz2, eps, eps_start, max_rounds)
    dev = xyz1.device
    assignment = torch.empty(B, n, device=dev, dtype=torch.int32)
    cost = torch.empty(B, n, device=dev, dtype=torch.float32)
    price = torch.empty(B, n, device=dev, dtype=torch.float32)
    emd = torch.empty(B, device=dev, dtype=torch.float64)
    rounds = torch.empty(B, device=dev, dtype=torch.int32)
    converged = torch.empty(B, device=dev, dtype=torch.int32)
    if B == 0:
        return EmdResult(assignment, cost, price, emd, rounds, converged)
    lib = _lib.load()
    eps_host = (ctypes.c_float * len(phases))(*phases)              # read by the entry point before it returns
    with torch.cuda.device(dev):
        code = lib.sc_emd3d_match(_lib.ptr(xyz1), _lib.ptr(xyz2), B, n, eps_host, len(phases), max_rounds, _lib.ptr(assignment),
                                  _lib.ptr(cost), _lib.ptr(price), _lib.ptr(rounds), _lib.ptr(converged), _lib.ptr(emd), _lib.stream())
    _lib.check(code, "sc_emd3d_match")
    return EmdResult(assignment, cost, price, emd, rounds, converged)


# ---- evaluation: per-triangle texture atlas (csrc/texture_bake.hip) --------------------------------------------------------------------
TEXTURE_TEXELS = (4, 32)            # the cell side T sc_texture_* take
TEXTURE_ATLAS = (64, 8192)          # the atlas side A: a power of two in this range
TEXTURE_MAX_IMAGES = 65535
TextureLayout = collections.namedtuple("TextureLayout", ["atlas", "cells", "rows"])


def texture_layout(f_max: int, texels: int) -> TextureLayout:
    """The atlas of a batch whose largest mesh has f_max faces, at `texels` = T texels per cell side: (A, n, rows) with A the smallest
    power of two in 64..8192 whose n = A // T cells per side hold ceil(f_max / 2) cells (two faces share a cell), and rows =
    T ceil(ceil(f_max / 2) / n), the atlas rows that hold a face.  ValueError when 8192 does not suffice (names eval.texture_texels)."""
    if isinstance(texels, bool) or not isinstance(texels, int) or not TEXTURE_TEXELS[0] <= texels <= TEXTURE_TEXELS[1]:
        raise ValueError("shapeclipper_amd: texture_layout: texels must be an integer in %d..%d, got %r" % (*TEXTURE_TEXELS, texels))
    if f_max < 0:
        raise ValueError("shapeclipper_amd: texture_layout: f_max must be >= 0, got %r" % (f_max,))
    cells = (int(f_max) + 1) // 2
    A = TEXTURE_ATLAS[0]
    while (A // texels) ** 2 < cells:
        A *= 2
        if A > TEXTURE_ATLAS[1]:
            raise ValueError("shapeclipper_amd: a mesh of %d faces does not fit an %d x %d atlas at eval.texture_texels = %d; lower "
                             "eval.texture_texels or eval.vox_res" % (f_max, TEXTURE_ATLAS[1], TEXTURE_ATLAS[1], texels))
    n = A // texels
    return TextureLayout(A, n, texels * ((cells + n - 1) // n))


def _texture_atlas_arg(who, A):
    if isinstance(A, bool) or not isinstance(A, int) or not TEXTURE_ATLAS[0] <= A <= TEXTURE_ATLAS[1] or A & (A - 1):
        raise ValueError("shapeclipper_amd: %s: the atlas side must be a power of two in %d..%d, got %r" % (who, *TEXTURE_ATLAS, A))


def texture_queries(verts, faces, v_start, f_start, f_count, A, T, lo, hi, S, rows, extra=0):
    """The network query point of every atlas texel: mesh.verts (grid-index units), mesh.faces and *mesh.starts() of a PackedMesh
    (mesh_pack.py) -- v_start / f_start / f_count sequences of B host integers: image b's faces are
    faces[f_start[b]:f_start[b] + f_count[b]], its vertex k is verts[v_start[b] + k] -> (query [B (rows A + extra), 3] fp32,
    face_of_texel [B, rows A] int32).  Image b's texel (x, y) is row y A + x of its block of rows A + extra query rows, the padded
    one-launch layout of sdf_forward / rgb_points_forward with n_per_image = rows A + extra; the `extra` rows behind the texels are
    left unwritten for the caller (eval_3D.mesh_texture puts the face centroids there).  A used texel is queried at
    lo + v (hi - lo) / (S - 1), v the affine map of its face at the texel's barycentrics; an unused one (face_of_texel -1) repeats the
    image's first texel.  include/shapeclipper_hip.h states layout and arithmetic (sc_texture_queries); texture_layout gives A and
    rows.  One launch on the current stream, no host synchronisation."""
    who = "texture_queries"
    verts, faces = check_mesh_tensors(who, verts, faces)
    _texture_atlas_arg(who, A)
    V, F = verts.shape[0], faces.shape[0]
    v_start, f_start, f_count = check_starts(who, v_start, f_start, f_count, V, F, TEXTURE_MAX_IMAGES)
    B = len(f_count)
    if isinstance(T, bool) or not isinstance(T, int) or not TEXTURE_TEXELS[0] <= T <= TEXTURE_TEXELS[1]:
        raise ValueError("shapeclipper_amd: texture_queries: T must be an integer in %d..%d, got %r" % (*TEXTURE_TEXELS, T))
    n = A // T
    for b in range(B):
        if f_count[b] > 2 * n * (rows // T):
            raise ValueError("shapeclipper_amd: texture_queries: image %d has %d faces; %d rows of an atlas of %d hold %d at T = %d"
                             % (b, f_count[b], rows, A, 2 * n * (rows // T), T))
    if not 0 <= rows <= A or rows % T or extra < 0 or S < 2:
        raise ValueError("shapeclipper_amd: texture_queries needs 0 <= rows <= A, rows a multiple of T, extra >= 0 and S >= 2")
    dev = verts.device
    stride = rows * A + extra
    query = torch.empty(B * stride, 3, device=dev, dtype=torch.float32)
    face_of_texel = torch.empty(B, rows * A, device=dev, dtype=torch.int32)
    if B == 0 or rows == 0:
        return query, face_of_texel
    starts = torch.tensor([v_start, f_start, f_count], dtype=torch.int64).to(dev)
    with torch.cuda.device(dev):
        code = _lib.load().sc_texture_queries(_lib.ptr(verts) if V else None, _lib.ptr(faces) if F else None, _lib.ptr(starts[0]),
                                              _lib.ptr(starts[1]), _lib.ptr(starts[2]), B, V, F, A, T, float(lo), float(hi), int(S), rows,
                                              stride, _lib.ptr(query), _lib.ptr(face_of_texel), _lib.stream())
    _lib.check(code, "sc_texture_queries")
    return query, face_of_texel


def texture_pack(rgb, normal, face_of_texel, A, rows):
    """rgb, normal [B rows A, 3] fp32 (the colours and unit normals at texture_queries' points, image after image) and face_of_texel
    [B, rows A] int32 -> (atlas, normal_atlas) uint8 [B, A, A, 3]: a used texel holds trunc(clamp(c, 0, 1) * 255) -- the recipe of the
    PNG dumps and of mesh_attributes -- and trunc(clamp((n + 1) / 2, 0, 1) * 255) of the object-space normal; texels without a face
    and the rows >= `rows` hold 127.  One launch (sc_texture_pack), no host synchronisation."""
    who = "texture_pack"
    _texture_atlas_arg(who, A)
    face_of_texel = device_tensor(who, "face_of_texel", face_of_texel, (torch.int32,))
    dev = face_of_texel.device
    rgb = device_tensor(who, "rgb", rgb, (torch.float32,), dev)
    normal = device_tensor(who, "normal", normal, (torch.float32,), dev)
    if not 0 <= rows <= A or face_of_texel.dim() != 2 or face_of_texel.shape[1] != rows * A:
        raise ValueError("shapeclipper_amd: texture_pack takes face_of_texel [B, rows A] with 0 <= rows <= A, got %s at rows = %r, A = %d"
                         % (tuple(face_of_texel.shape), rows, A))
    B = face_of_texel.shape[0]
    if B > TEXTURE_MAX_IMAGES or tuple(rgb.shape) != (B * rows * A, 3) or tuple(normal.shape) != (B * rows * A, 3):
        raise ValueError("shapeclipper_amd: texture_pack takes rgb and normal [B rows A, 3] = [%d, 3] for at most %d images, got %s and %s"
                         % (B * rows * A, TEXTURE_MAX_IMAGES, tuple(rgb.shape), tuple(normal.shape)))
    atlas = torch.empty(B, A, A, 3, device=dev, dtype=torch.uint8)
    atlas_n = torch.empty(B, A, A, 3, device=dev, dtype=torch.uint8)
    if B == 0:
        return atlas, atlas_n
    live = rows > 0
    with torch.cuda.device(dev):
        code = _lib.load().sc_texture_pack(_lib.ptr(rgb) if live else None, _lib.ptr(normal) if live else None,
                                           _lib.ptr(face_of_texel) if live else None, B, A, rows, _lib.ptr(atlas), _lib.ptr(atlas_n),
                                           _lib.stream())
    _lib.check(code, "sc_texture_pack")
    return atlas, atlas_n


def texture_sample(atlas, uv, image_of_point):
    """The bilinear look-up a viewer performs: atlas [B, A, A, C] fp32 or uint8 (read as float, not scaled), uv [N, 2] fp32 in the OBJ
    convention (u to the right, v upward, texel centres at (k + 0.5) / A), image_of_point [N] int32 -> [N, C] fp32.  Indices clamp to the
    atlas edge; include/shapeclipper_hip.h states the expression (sc_texture_sample).  One launch, no host synchronisation."""
    who = "texture_sample"
    atlas = device_tensor(who, "atlas", atlas, (torch.float32, torch.uint8))
    dev = atlas.device
    uv = device_tensor(who, "uv", uv, (torch.float32,), dev)
    image_of_point = device_tensor(who, "image_of_point", image_of_point, (torch.int32,), dev)
    if atlas.dim() != 4 or atlas.shape[1] != atlas.shape[2] or not 1 <= atlas.shape[3] <= 16 or atlas.shape[0] < 1:
        raise ValueError("shapeclipper_amd: texture_sample takes an atlas [B, A, A, C] with B >= 1 and 1 <= C <= 16, got %s" % (tuple(atlas.shape),))
    B, A, C = atlas.shape[0], atlas.shape[1], atlas.shape[3]
    _texture_atlas_arg(who, A)
    N = uv.shape[0]
    if B > TEXTURE_MAX_IMAGES or tuple(uv.shape) != (N, 2) or tuple(image_of_point.shape) != (N,):
        raise ValueError("shapeclipper_amd: texture_sample takes uv [N, 2] and image_of_point [N], got %s and %s"
                         % (tuple(uv.shape), tuple(image_of_point.shape)))
    out = torch.empty(N, C, device=dev, dtype=torch.float32)
    if N == 0:
        return out
    with torch.cuda.device(dev):
        code = _lib.load().sc_texture_sample(_lib.ptr(atlas), 1 if atlas.dtype == torch.uint8 else 0, _lib.ptr(uv), _lib.ptr(image_of_point),
                                             N, B, A, C, _lib.ptr(out), _lib.stream())
    _lib.check(code, "sc_texture_sample")
    return out


# ---- evaluation: triangle rasteriser (csrc/mesh_raster.hip) -----------------------------------------------------------------------------
RASTER_MAX_SIDE = 4096
RASTER_MAX_VIEWS = 65535
RASTER_MAX_IMAGES = 65535
RASTER_LARGE_PIXELS = 64            # a face whose box holds more pixel centres is walked by a wave, not by its own thread
MeshRaster = collections.namedtuple("MeshRaster", ["face", "depth", "bary", "stats"])


def mesh_raster(verts, faces, v_start, f_start, f_count, pose, intr, H, W, near, large_pixels=RASTER_LARGE_PIXELS):
    """The PackedMesh (mesh_pack.py) of B images, each seen from n_views cameras: verts [V,3] fp32 in world units, mesh.faces and
    *mesh.starts() -- v_start / f_start / f_count sequences of B host integers as texture_queries takes them, the images in order (image
    b's vertices are verts[v_start[b]:v_start[b + 1]], the last image's run to V) --, pose [B, n_views, 3, 4] world-to-camera (camera.world2cam's
    convention), intr [B, 3, 3] -> MeshRaster(face [B, n_views, H, W] int32 -- the image's face nearest to the camera at the pixel's
    centre, -1 where none covers it --, depth [B, n_views, H, W] fp32 camera z (0 on a miss), bary [B, n_views, H, W, 3] fp32
    perspective-correct barycentrics (0 on a miss), stats [B, n_views, 4] int32: faces drawn, culled by `near`, culled by range or not
    finite, of zero area).  A face with a vertex nearer than `near` is dropped whole (no clipping); rendering is two-sided.
    include/shapeclipper_hip.h states the arithmetic (sc_mesh_raster): integer coverage with the top-left rule on a 1/256-pixel
    lattice, visibility by a 64-bit integer atomicMin, the same bits from run to run.  large_pixels chooses between the two coverage
    paths, which agree bit for bit.  Scratch from the `_scratch` cache (tag "mesh_raster"); three memsets and four launches on the
    current stream, no host synchronisation."""
    who = "mesh_raster"
    verts, faces = check_mesh_tensors(who, verts, faces)
    dev = verts.device
    pose = device_tensor(who, "pose", pose, (torch.float32,), dev)
    intr = device_tensor(who, "intr", intr, (torch.float32,), dev)
    V, F = verts.shape[0], faces.shape[0]
    v_start, f_start, f_count = check_starts(who, v_start, f_start, f_count, V, F, RASTER_MAX_IMAGES)
    B = len(f_count)
    if pose.dim() != 4 or pose.shape[0] != B or tuple(pose.shape[2:]) != (3, 4) or not 1 <= pose.shape[1] <= RASTER_MAX_VIEWS:
        raise ValueError("shapeclipper_amd: mesh_raster takes pose [B, n_views, 3, 4] with B = %d and 1 <= n_views <= %d, got %s"
                         % (B, RASTER_MAX_VIEWS, tuple(pose.shape)))
    if tuple(intr.shape) != (B, 3, 3):
        raise ValueError("shapeclipper_amd: mesh_raster takes intr [B, 3, 3] with B = %d, got %s" % (B, tuple(intr.shape)))
    for name, v in (("H", H), ("W", W)):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= RASTER_MAX_SIDE:
            raise ValueError("shapeclipper_amd: mesh_raster: %s must be an integer in 1..%d, got %r" % (name, RASTER_MAX_SIDE, v))
    if isinstance(near, bool) or not isinstance(near, (int, float)) or not near > 0:
        raise ValueError("shapeclipper_amd: mesh_raster: near must be a positive number, got %r" % (near,))
    if isinstance(large_pixels, bool) or not isinstance(large_pixels, int) or large_pixels < 0:
        raise ValueError("shapeclipper_amd: mesh_raster: large_pixels must be an integer >= 0, got %r" % (large_pixels,))
    n_views = pose.shape[1]
    for b in range(B):
        v_end = v_start[b + 1] if b + 1 < B else V
        if not 0 <= v_start[b] <= v_end <= V:
            raise ValueError("shapeclipper_amd: mesh_raster: v_start must be non-decreasing within 0..%d, got %r" % (V, v_start))
        if b and f_start[b] < f_start[b - 1] + f_count[b - 1]:
            raise ValueError("shapeclipper_amd: mesh_raster: image %d's faces f_start + [0, f_count) = [%d, %d) overlap the image before"
                             % (b, f_start[b], f_start[b] + f_count[b]))
        if f_count[b] > 0 and v_end == v_start[b]:
            raise ValueError("shapeclipper_amd: mesh_raster: image %d has %d faces and no vertex" % (b, f_count[b]))
    lib = _lib.load()
    n_bytes = lib.sc_mesh_raster_scratch_bytes(B, n_views, V, F, H, W)
    if n_bytes < 0:
        raise ValueError("shapeclipper_amd: mesh_raster: %d images x %d views of %d x %d pixels are more than one call takes" % (B, n_views, H, W))
    if B == 0 or V == 0 or F == 0:          # nothing to draw: every pixel a miss
        return MeshRaster(torch.full((B, n_views, H, W), -1, device=dev, dtype=torch.int32), torch.zeros(B, n_views, H, W, device=dev),
                          torch.zeros(B, n_views, H, W, 3, device=dev), torch.zeros(B, n_views, 4, device=dev, dtype=torch.int32))
    out = MeshRaster(torch.empty(B, n_views, H, W, device=dev, dtype=torch.int32), torch.empty(B, n_views, H, W, device=dev),
                     torch.empty(B, n_views, H, W, 3, device=dev), torch.empty(B, n_views, 4, device=dev, dtype=torch.int32))
    ws = _scratch("mesh_raster", dev, (n_bytes + 3) // 4)
    starts = torch.tensor([v_start, f_start, f_count], dtype=torch.int64).to(dev)
    with torch.cuda.device(dev):
        code = lib.sc_mesh_raster(_lib.ptr(verts), _lib.ptr(faces), _lib.ptr(starts[0]), _lib.ptr(starts[1]), _lib.ptr(starts[2]),
                                  _lib.ptr(pose), _lib.ptr(intr), B, V, F, n_views, H, W, float(near), int(large_pixels),
                                  _lib.ptr(out.face), _lib.ptr(out.depth), _lib.ptr(out.bary), _lib.ptr(out.stats), _lib.ptr(ws),
                                  _lib.stream())
    _lib.check(code, "sc_mesh_raster")
    return out


# ---- evaluation: volumetric IoU of two point clouds from voxel solids (csrc/voxel_solid.hip) ------------------------------------------
VOXEL_MIN_RES = 8               # SC_VOXEL_MIN_RES
VOXEL_MAX_RES = 64              # SC_VOXEL_MAX_RES
VOXEL_MAX_CLOSE = 2             # SC_VOXEL_MAX_CLOSE
VOXEL_MAX_IMAGES = 65535
VOXEL_MAX_WORDS = 1 << 24
VoxelSolid = collections.namedtuple("VoxelSolid", ["bits", "shell_voxels", "solid_voxels", "sweeps"])


def _voxel_grid(who, res, close):
    """ValueError unless res is an integer in 8..64 and close an integer in 0..2."""
    if isinstance(res, bool) or not isinstance(res, int) or not VOXEL_MIN_RES <= res <= VOXEL_MAX_RES:
        raise ValueError("%s: res must be an integer in %d..%d, got %r" % (who, VOXEL_MIN_RES, VOXEL_MAX_RES, res))
    if isinstance(close, bool) or not isinstance(close, int) or not 0 <= close <= VOXEL_MAX_CLOSE:
        raise ValueError("%s: close must be an integer in 0..%d, got %r" % (who, VOXEL_MAX_CLOSE, close))


def _voxel_args(who, tensors, dtype, check):
    """The checks of the voxel entry points, in _emd_args' order: TypeError for something that is not a tensor of `dtype`, then
    check() (ValueError for shapes, sizes and settings) -- all before the device is looked at -- then RuntimeError for host tensors
    and ValueError for another device or a non-contiguous tensor.  tensors: ((name, tensor), ...)."""
    for name, t in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a tensor, got %s" % (who, name, type(t).__name__))
        if t.dtype != dtype:
            raise TypeError("%s: %s must be %s, got %s" % (who, name, dtype, t.dtype))
    check()
    if not all(t.is_cuda for _, t in tensors):
        raise RuntimeError(_lib.NO_CPU)
    first = tensors[0]
    for name, t in tensors[1:]:
        if t.device != first[1].device:
            raise ValueError("%s: %s is on %s, %s is on %s" % (who, name, t.device, first[0], first[1].device))
    for name, t in tensors:
        if not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous" % (who, name))


def voxel_frame(a, b, res=32, close=1):
    """a [B,N,3], b [B,M,3] fp32 (N, M >= 1), res in 8..64, close in 0..2 -> (origin [B,3], pitch [B]) fp32: the frame the two clouds
    share as res^3 voxels -- the cube around their common bounding box, close + 1 empty layers on every side (include/
    shapeclipper_hip.h, sc_voxel_frame, states the expression).  Coincident clouds get pitch 1; a coordinate that is not finite makes
    the image's origin and pitch NaN.

    Host synchronisation: none.  Runs on the current stream."""
    who = "shapeclipper_amd: voxel_frame"

    def check():
        if a.dim() != 3 or b.dim() != 3 or a.shape[2] != 3 or b.shape[2] != 3 or a.shape[0] != b.shape[0]:
            raise ValueError("%s: a and b must be [B,N,3] and [B,M,3], got %s and %s" % (who, tuple(a.shape), tuple(b.shape)))
        if a.shape[1] < 1 or b.shape[1] < 1:
            raise ValueError("%s: a cloud needs at least one point, got %d and %d" % (who, a.shape[1], b.shape[1]))
        if a.shape[0] > VOXEL_MAX_IMAGES:
            raise ValueError("%s takes at most %d images per call, got %d" % (who, VOXEL_MAX_IMAGES, a.shape[0]))
        _voxel_grid(who, res, close)
    _voxel_args(who, (("a", a), ("b", b)), torch.float32, check)
    B = a.shape[0]
    origin = torch.empty(B, 3, device=a.device, dtype=torch.float32)
    pitch = torch.empty(B, device=a.device, dtype=torch.float32)
    if B == 0:
        return origin, pitch
    lib = _lib.load()
    with torch.cuda.device(a.device):
        code = lib.sc_voxel_frame(_lib.ptr(a), _lib.ptr(b), B, a.shape[1], b.shape[1], res, close, _lib.ptr(origin), _lib.ptr(pitch),
                                  _lib.stream())
    _lib.check(code, "sc_voxel_frame")
    return origin, pitch


def voxel_solid(points, origin, pitch, res=32, close=1):
    """points [B,N,3], origin [B,3], pitch [B] fp32 -> VoxelSolid(bits [B,res,res] int64, shell_voxels [B], solid_voxels [B], sweeps [B]
    int32): the solid of a point cloud in the frame (origin, pitch) of res^3 voxels.  Bit z of bits[b, x, y] is voxel (x, y, z).  The
    points are splatted to a voxel shell (shell_voxels of them), the shell is dilated `close` times by the 3x3x3 cube, the space the
    exterior cannot reach through 6-neighbours is filled, and the result is eroded `close` times: scipy.ndimage's
    binary_erosion(binary_fill_holes(binary_dilation(shell))).  sweeps counts the Jacobi sweeps of the exterior flood.  A point with
    a coordinate that is not finite sets nothing; a frame that is not finite gives the empty solid.  One workgroup per image, the
    whole job in LDS (csrc/voxel_solid.hip); the same bits from run to run, alone or in a batch.  No gradient.

    Host synchronisation: none.  Runs on the current stream."""
    who = "shapeclipper_amd: voxel_solid"

    def check():
        if points.dim() != 3 or points.shape[2] != 3:
            raise ValueError("%s: points must be [B,N,3], got %s" % (who, tuple(points.shape)))
        B = points.shape[0]
        if tuple(origin.shape) != (B, 3) or tuple(pitch.shape) != (B,):
            raise ValueError("%s: origin and pitch must be [%d,3] and [%d], got %s and %s" % (who, B, B, tuple(origin.shape), tuple(pitch.shape)))
        if points.shape[1] < 1:
            raise ValueError("%s: a cloud needs at least one point" % who)
        if B > VOXEL_MAX_IMAGES:
            raise ValueError("%s takes at most %d images per call, got %d" % (who, VOXEL_MAX_IMAGES, B))
        _voxel_grid(who, res, close)
    _voxel_args(who, (("points", points), ("origin", origin), ("pitch", pitch)), torch.float32, check)
    B, dev = points.shape[0], points.device
    bits = torch.empty(B, res, res, device=dev, dtype=torch.int64)
    shell, solid, sweeps = (torch.empty(B, device=dev, dtype=torch.int32) for _ in range(3))
    if B == 0:
        return VoxelSolid(bits, shell, solid, sweeps)
    lib = _lib.load()
    with torch.cuda.device(dev):
        code = lib.sc_voxel_solid(_lib.ptr(points), _lib.ptr(origin), _lib.ptr(pitch), B, points.shape[1], res, close, _lib.ptr(bits),
                                  _lib.ptr(shell), _lib.ptr(solid), _lib.ptr(sweeps), _lib.stream())
    _lib.check(code, "sc_voxel_solid")
    return VoxelSolid(bits, shell, solid, sweeps)


def voxel_iou(bits_a, bits_b):
    """bits_a, bits_b [B,...] int64 of one shape (bit volumes, voxel_solid's bits) -> (inter [B], union [B]) int32: the voxels in both
    and the voxels in either.  The IoU is inter / union, 1 for an empty union (mask_iou's convention); the division is the caller's.

    Host synchronisation: none.  Runs on the current stream."""
    who = "shapeclipper_amd: voxel_iou"

    def check():
        if bits_a.dim() < 2 or tuple(bits_a.shape) != tuple(bits_b.shape):
            raise ValueError("%s: bits_a and bits_b must have one shape [B,...], got %s and %s" % (who, tuple(bits_a.shape), tuple(bits_b.shape)))
        words = bits_a[0].numel() if bits_a.shape[0] else 1
        if not 1 <= words <= VOXEL_MAX_WORDS:
            raise ValueError("%s: 1..%d words per image, got %d" % (who, VOXEL_MAX_WORDS, words))
        if bits_a.shape[0] > VOXEL_MAX_IMAGES:
            raise ValueError("%s takes at most %d images per call, got %d" % (who, VOXEL_MAX_IMAGES, bits_a.shape[0]))
    _voxel_args(who, (("bits_a", bits_a), ("bits_b", bits_b)), torch.int64, check)
    B, dev = bits_a.shape[0], bits_a.device
    inter = torch.empty(B, device=dev, dtype=torch.int32)
    union = torch.empty(B, device=dev, dtype=torch.int32)
    if B == 0:
        return inter, union
    lib = _lib.load()
    with torch.cuda.device(dev):
        code = lib.sc_voxel_iou(_lib.ptr(bits_a), _lib.ptr(bits_b), B, bits_a[0].numel(), _lib.ptr(inter), _lib.ptr(union), _lib.stream())
    _lib.check(code, "sc_voxel_iou")
    return inter, union


# ---- evaluation: topology, area and volume of indexed triangle meshes (csrc/mesh_topology.hip) -----------------------------------------
MESH_TOPOLOGY_MAX_IMAGES = 65535
MESH_TOPOLOGY_MAX_FACES = 1 << 26
MESH_TOPOLOGY_MAX_SLOTS = 1 << 30
MESH_TOPOLOGY_COUNTS = ("vertices", "unreferenced_vertices", "faces", "degenerate_faces", "edges", "boundary_edges", "nonmanifold_edges",
                        "inconsistent_edges", "components", "largest_component_faces", "nonmanifold_vertices", "euler", "genus")
MESH_TOPOLOGY_FLAGS = ("watertight", "oriented", "manifold")        # rows 13..15 of sc_mesh_topology's counts (SC_MESH_TOPOLOGY_FIELDS = 16)
MeshTopology = collections.namedtuple("MeshTopology", MESH_TOPOLOGY_COUNTS + MESH_TOPOLOGY_FLAGS + ("area", "volume", "face_component"))


def mesh_topology_slots(n_faces: int) -> int:
    """The default size of mesh_topology's edge table: the smallest power of two >= 6 n_faces + 2, twice the half-edges and more."""
    return 1 << (6 * n_faces + 1).bit_length()


def _edge_table_slots(who, n_faces, table_slots, default=True):
    """table_slots, validated for a mesh of n_faces faces; for None, the default size (or None where the caller sizes the table later)."""
    if table_slots is None:
        return mesh_topology_slots(n_faces) if default else None
    if (isinstance(table_slots, bool) or not isinstance(table_slots, int) or table_slots < 1 or table_slots & (table_slots - 1)
            or table_slots <= 3 * n_faces or table_slots > MESH_TOPOLOGY_MAX_SLOTS):
        raise ValueError("%s: table_slots must be a power of two greater than 3 F = %d (and at most 2^30), got %r"
                         % (who, 3 * n_faces, table_slots))
    return table_slots


def _finite_number(x):
    return isinstance(x, (int, float)) and not isinstance(x, bool) and x == x and abs(x) != float("inf")


def mesh_topology(verts, faces, v_count, f_count, table_slots=None):
    """A PackedMesh (mesh_pack.py) of B images, passed as `*mesh` -- verts and faces on the device, v_count / f_count [B] int64 or int32,
    on the host (as every producer returns them) or on the device -> MeshTopology of [B] int64 device tensors vertices (referenced
    ones), unreferenced_vertices,
    faces (non-degenerate), degenerate_faces, edges, boundary_edges (one face), nonmanifold_edges (three or more), inconsistent_edges
    (two faces that traverse the edge the same way), components (what trimesh.split returns), largest_component_faces,
    nonmanifold_vertices (more than one fan of corners), euler = V - E + F and genus (components - euler / 2 for a watertight, oriented,
    manifold mesh with faces; -1 otherwise); [B] bool watertight, oriented, manifold; [B] float64 area and signed volume (fixed-order
    sums); and face_component [F] int32, the lowest local face number of the face's component (-1 for a degenerate face).
    include/shapeclipper_hip.h states every rule (sc_mesh_topology); tests/mesh_topology_ref.py restates them in numpy.  An image
    without faces gets zeros, genus -1 and the flags as defined (all true).

    The edges are matched in an open-addressing table of `table_slots` slots in the scratch cache ("mesh topology"): a power of two
    greater than 3 F, by default mesh_topology_slots(F) >= 6 F (for tests: no output depends on it).  Integer atomics only decide the
    integer outputs and no float is accumulated by an atomic: the same bits from run to run, for any batch and stream.

    ValueError for wrong dtypes, shapes or devices, counts that are negative or do not sum to the packed lengths, a bad table_slots --
    all before any launch -- and for a face index outside its image's vertex range: that is checked on the device (such a face is
    never dereferenced) and raised after the launches.

    Host synchronisation: one read of a 4-byte flag after the launches (the index check).  Runs on the current stream."""
    who = "shapeclipper_amd: mesh_topology"
    B, V, F, _, offsets = check_packed(who, verts, faces, v_count, f_count, max_images=MESH_TOPOLOGY_MAX_IMAGES,
                                       max_faces=MESH_TOPOLOGY_MAX_FACES)
    dev = verts.device
    table_slots = _edge_table_slots(who, F, table_slots)
    counts = torch.empty(len(MESH_TOPOLOGY_COUNTS) + len(MESH_TOPOLOGY_FLAGS), B, device=dev, dtype=torch.int64)
    measures = torch.empty(2, B, device=dev, dtype=torch.float64)
    face_component = torch.empty(F, device=dev, dtype=torch.int32)
    if B > 0:
        offsets = offsets.to(dev)
        bad = torch.empty(1, device=dev, dtype=torch.int32)
        lib = _lib.load()
        with torch.cuda.device(dev):
            ws = _scratch("mesh topology", dev, (lib.sc_mesh_topology_scratch_bytes(B, V, F, table_slots) + 3) // 4)
            code = lib.sc_mesh_topology(_lib.ptr(verts.contiguous()) if V else None, _lib.ptr(faces.contiguous()) if F else None,
                                        _lib.ptr(offsets[0]), _lib.ptr(offsets[1]), B, V, F, table_slots, _lib.ptr(ws), _lib.ptr(counts),
                                        _lib.ptr(measures[0]), _lib.ptr(measures[1]), _lib.ptr(face_component) if F else None,
                                        _lib.ptr(bad), _lib.stream())
        _lib.check(code, "sc_mesh_topology")
        if int(bad.item()):
            raise ValueError("%s: a face index lies outside its image's vertex range [0, v_count[b])" % who)
    n = len(MESH_TOPOLOGY_COUNTS)
    return MeshTopology(*counts[:n].unbind(0), *(counts[n + k] != 0 for k in range(len(MESH_TOPOLOGY_FLAGS))), measures[0], measures[1],
                        face_component)


# ---- validity: pairs of faces that properly cross (csrc/mesh_intersect.hip) --------------------------------------------------------------
MESH_INTERSECT_MAX_IMAGES = 65535
MESH_INTERSECT_MAX_FACES = 1 << 26
MeshIntersections = collections.namedtuple("MeshIntersections", ["pairs", "pairs_vertex", "box_pairs", "faces_hit", "degenerate", "hits",
                                                                 "partner"])


def mesh_self_intersections(verts, faces, v_count, f_count, search="grid"):
    """A PackedMesh (mesh_pack.py) of B images, passed as `*mesh` -- verts and faces on the device, v_count / f_count [B] int64 or int32,
    on the host (as every producer returns them) or on the device -> MeshIntersections, all on the device: pairs [B] int64, the pairs of
    faces of an image that properly cross; pairs_vertex [B] int64, those of them that share one vertex; box_pairs [B] int64, the pairs
    that share at most one index and whose closed fp32 boxes overlap (the candidates: a function of the mesh alone, whatever the
    search); faces_hit [B] int32, the faces in at least one such pair; degenerate [B] int32, the faces that repeat an index (they take
    part in nothing); hits [F] int32, per packed face how many faces it crosses; partner [F] int32, the lowest image-local face it
    crosses, or -1.  include/shapeclipper_hip.h states the rule (sc_mesh_self_intersections); tests/mesh_intersect_ref.py restates it in
    numpy.  The rule is STRICT: a filtered float64 orientation sign that is either zero or the sign of the exact determinant, so every
    counted pair truly intersects, and contacts with a zero sign -- a vertex on a face, an edge through an edge, coplanar overlap -- are
    not counted: the count is a lower bound.  Faces that share two or three indices are never a pair.
    search="grid": the triangle grid of point_mesh_distance (csrc/triangle_grid.hpp), every candidate pair tested once; search="brute":
    all pairs, the same integers.  Integer atomics only: the same bits from run to run, for any batch, stream and face order.

    ValueError for wrong dtypes, shapes or devices, counts that are negative or do not sum to the packed lengths, a bad search -- all
    before any launch -- and for a vertex that is not finite or of magnitude 1e15 or more and for a face index outside its image's vertex
    range: both are flagged on the device (such a face is never dereferenced) and raised after the launches.

    Host synchronisation: one read of the two 4-byte flags after the launches.  Runs on the current stream; the workspace has a fixed
    capacity (the `_scratch` cache, tag "mesh intersect")."""
    who = "shapeclipper_amd: mesh_self_intersections"
    if search not in ("grid", "brute"):
        raise ValueError("%s: search must be 'grid' or 'brute', got %r" % (who, search))
    B, V, F, counts_host, _ = check_packed(who, verts, faces, v_count, f_count, max_images=MESH_INTERSECT_MAX_IMAGES,
                                           max_faces=MESH_INTERSECT_MAX_FACES)
    dev = verts.device
    counts = torch.zeros(3, B, device=dev, dtype=torch.int64)
    face_counts = torch.zeros(2, B, device=dev, dtype=torch.int32)
    hits = torch.empty(F, device=dev, dtype=torch.int32)
    partner = torch.empty(F, device=dev, dtype=torch.int32)
    if B > 0:
        counts32 = counts_host.int().to(dev)                            # the C entry point takes int32 device counts
        flags = torch.empty(2, device=dev, dtype=torch.int32)
        lib = _lib.load()
        with torch.cuda.device(dev):
            ws = _scratch("mesh intersect", dev, (lib.sc_mesh_self_intersections_scratch_bytes(B, V, F) + 3) // 4)
            code = lib.sc_mesh_self_intersections(_lib.ptr(verts.contiguous()) if V else None, _lib.ptr(faces.contiguous()) if F else None,
                                                  _lib.ptr(counts32[0]), _lib.ptr(counts32[1]), B, V, F, 1 if search == "brute" else 0,
                                                  _lib.ptr(ws), _lib.ptr(counts), _lib.ptr(face_counts), _lib.ptr(hits) if F else None,
                                                  _lib.ptr(partner) if F else None, _lib.ptr(flags), _lib.stream())
        _lib.check(code, "sc_mesh_self_intersections")
        bad_vertex, bad_index = flags.tolist()
        if bad_vertex:
            raise ValueError("%s: a vertex is not finite or has a magnitude of 1e15 or more" % who)
        if bad_index:
            raise ValueError("%s: a face index lies outside its image's vertex range [0, v_count[b])" % who)
    return MeshIntersections(counts[0], counts[1], counts[2], face_counts[0], face_counts[1], hits, partner)


# ---- evaluation: decimation by vertex clustering with quadric placement (csrc/mesh_simplify.hip) ----------------------------------------
MESH_SIMPLIFY_MAX_CELLS = 128               # SC_MESH_SIMPLIFY_MAX_CELLS
MESH_SIMPLIFY_MAX_WORDS = 1 << 28           # mask words of a whole batch: B ceil(G^3 / 64)


class SimplifiedMesh(collections.namedtuple("SimplifiedMesh", ["verts", "faces", "v_count", "f_count", "vertex_cluster", "face_source",
                                                               "collapsed", "cancelled"])):
    __slots__ = ()
    packed = property(lambda self: PackedMesh(*self[:4]), doc="the simplified meshes alone, as a PackedMesh")


def mesh_cluster_simplify(verts, faces, v_count, f_count, origin, pitch, cells, reg=0.05):
    """Decimates a PackedMesh (mesh_pack.py) of B images, passed as `*mesh` -- verts and faces on the device, v_count / f_count [B] int64
    or int32 (host or device) -- by vertex clustering.  A box of `cells` = G cells per axis (1..128) of side `pitch` > 0 with its lower corner at `origin` (three numbers) is laid
    over every image, the vertices of a cell become one vertex at the minimiser of the cell's quadric (the planes of the faces that
    touch it, regularised towards the mean of its vertices by `reg` > 0, clamped into the cell), faces with two corners in one cell
    collapse, and of the faces left on one cluster triple opposite ones cancel and like-oriented copies leave one.
    include/shapeclipper_hip.h states every rule (sc_mesh_cluster_simplify); tests/mesh_simplify_ref.py restates them in numpy.

    -> SimplifiedMesh(verts [V',3] fp32, faces [F',3] int32 image-local, v_count, f_count [B] int64 on the host -- `.packed` is these
    four as a PackedMesh again, for mesh_topology, point_mesh_distance or this op --, vertex_cluster [V] int32 (old vertex -> new vertex
    of its image), face_source [F'] int32 (new face -> image-local old face), collapsed, cancelled [B] int64 on the device).  Output faces keep
    the source order; a cluster whose faces all vanished stays as an unreferenced vertex.  Only integer atomics decide anything: the
    same bits from run to run, for any batch, stream and face order.  Scratch comes from the scratch cache ("mesh simplify").

    ValueError for wrong dtypes, shapes or devices, counts that are negative or do not sum to the packed lengths, a bad origin, pitch,
    cells or reg -- all before any launch -- and, checked on the device and raised after the launches, for a vertex that is not finite
    or lies outside the box [origin, origin + G pitch] and for a face index outside its image's vertex range (neither is dereferenced).

    Host synchronisation: one read of the two flags and the per-image counts, which sizes the outputs.  Runs on the current stream."""
    who = "shapeclipper_amd: mesh_cluster_simplify"
    B, V, F, counts_host, offsets = check_packed(who, verts, faces, v_count, f_count, max_images=MESH_TOPOLOGY_MAX_IMAGES,
                                                 max_faces=MESH_TOPOLOGY_MAX_FACES)
    dev = verts.device
    if isinstance(origin, torch.Tensor):
        origin = origin.detach().cpu().reshape(-1).tolist()
    if not isinstance(origin, (list, tuple)) or len(origin) != 3 or not all(_finite_number(x) for x in origin):
        raise ValueError("%s: origin must be three finite numbers, got %r" % (who, origin))
    if not _finite_number(pitch) or not pitch > 0 or not float(torch.tensor(float(pitch), dtype=torch.float32)) > 0:
        raise ValueError("%s: pitch must be a finite number > 0 (as fp32), got %r" % (who, pitch))
    if isinstance(cells, bool) or not isinstance(cells, int) or not 1 <= cells <= MESH_SIMPLIFY_MAX_CELLS:
        raise ValueError("%s: cells must be an integer in 1..%d, got %r" % (who, MESH_SIMPLIFY_MAX_CELLS, cells))
    if not _finite_number(reg) or not reg > 0:
        raise ValueError("%s: reg must be a finite number > 0, got %r" % (who, reg))
    if B * ((cells ** 3 + 63) // 64) > MESH_SIMPLIFY_MAX_WORDS:
        raise ValueError("%s takes B ceil(cells^3 / 64) <= 2^28 mask words per call, got B = %d and cells = %d" % (who, B, cells))
    verts_out = torch.empty(V, 3, device=dev, dtype=torch.float32)
    faces_out = torch.empty(F, 3, device=dev, dtype=torch.int32)
    vertex_cluster = torch.empty(V, device=dev, dtype=torch.int32)
    face_source = torch.empty(F, device=dev, dtype=torch.int32)
    back = torch.zeros(4 * B + 1, device=dev, dtype=torch.int64)                    # what the host reads: the counts, then the two flags
    counts, bad = back[:4 * B].view(4, B), back[4 * B:].view(torch.int32)           # SC_MESH_SIMPLIFY_FIELDS rows; bad_vertex, bad_index
    if B == 0:
        return SimplifiedMesh(verts_out, faces_out, counts_host[0], counts_host[1], vertex_cluster, face_source, counts[2], counts[3])
    offsets = offsets.to(dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = _scratch("mesh simplify", dev, (lib.sc_mesh_cluster_simplify_scratch_bytes(B, V, F, cells) + 3) // 4)
        code = lib.sc_mesh_cluster_simplify(_lib.ptr(verts.contiguous()) if V else None, _lib.ptr(faces.contiguous()) if F else None,
                                            _lib.ptr(offsets[0]), _lib.ptr(offsets[1]), B, V, F, float(origin[0]), float(origin[1]),
                                            float(origin[2]), float(pitch), cells, float(reg), _lib.ptr(ws),
                                            _lib.ptr(verts_out) if V else None, _lib.ptr(faces_out) if F else None, _lib.ptr(counts),
                                            _lib.ptr(vertex_cluster) if V else None, _lib.ptr(face_source) if F else None,
                                            _lib.ptr(bad[:1]), _lib.ptr(bad[1:]), _lib.stream())
    _lib.check(code, "sc_mesh_cluster_simplify")
    host = back.cpu()
    flags, sizes = host[4 * B:].view(torch.int32).tolist(), host[:2 * B].view(2, B)
    if flags[0]:
        raise ValueError("%s: a vertex is not finite or lies outside the box [origin, origin + cells * pitch]" % who)
    if flags[1]:
        raise ValueError("%s: a face index lies outside its image's vertex range [0, v_count[b])" % who)
    return SimplifiedMesh(verts_out[:int(sizes[0].sum())], faces_out[:int(sizes[1].sum())], sizes[0], sizes[1], vertex_cluster,
                          face_source[:int(sizes[1].sum())], counts[2], counts[3])


# ---- post-processing: Taubin smoothing of indexed triangle meshes by the umbrella operator (csrc/mesh_smooth.hip) -----------------------
MESH_SMOOTH_MAX_ITERS = 1000                # SC_MESH_SMOOTH_MAX_ITERS
MESH_SMOOTH_MAX_VERTS = 1 << 30
MESH_SMOOTH_MU = 1.0 / (0.1 - 1.0 / 0.5)    # Taubin's mu for the pass-band 0.1 at lam = 0.5: -0.5263157894736842
MESH_SMOOTH_COUNTS = ("free", "fixed_boundary", "isolated", "degree_max")           # rows of sc_mesh_smooth's counts
MESH_SMOOTH_MEASURES = ("disp_mean", "disp_max", "rough_before", "rough_after")     # SmoothedMesh's order; the rows are 2, 3, 0, 1


class SmoothedMesh(collections.namedtuple("SmoothedMesh", ("verts", "faces", "v_count", "f_count") + MESH_SMOOTH_COUNTS + MESH_SMOOTH_MEASURES)):
    __slots__ = ()
    packed = property(lambda self: PackedMesh(*self[:4]), doc="the smoothed meshes alone, as a PackedMesh")


def mesh_smooth(verts, faces, v_count, f_count, iters, lam=0.5, mu=MESH_SMOOTH_MU, table_slots=None):
    """Smooths a PackedMesh (mesh_pack.py) of B images, passed as `*mesh` -- verts and faces on the device, v_count / f_count [B] int64 or
    int32 (host or device) -- by Taubin's lambda|mu scheme on the umbrella operator: `iters` (0..1000) iterations, each a Jacobi half-step
    x_i += lam (m_i - x_i) and, unless mu == 0 (plain Laplacian smoothing), a half-step with `mu` in [-1, 0]; m_i is the mean of the
    vertices that share an edge with i.  Vertices on an edge that one face only uses (the open rim) and vertices without a neighbour keep
    their bits; the faces are not changed.  The state is float64, every operation rounded once, the sums in ascending neighbour number;
    the output is rounded to fp32 once.  include/shapeclipper_hip.h states every rule (sc_mesh_smooth); tests/mesh_smooth_ref.py restates
    them in numpy.  The default mu is Taubin's for a pass-band of 0.1 at lam = 0.5.

    -> SmoothedMesh(verts [V,3] fp32, faces, v_count, f_count as given -- `.packed` is these four as a PackedMesh --, free,
    fixed_boundary, isolated, degree_max [B] int64 and disp_mean, disp_max (how far the free vertices moved), rough_before, rough_after
    (their mean |m_i - x_i| on the start and on the final state) [B] float64, all on the device, the measures fixed-order sums in the
    units of verts).  An image without faces returns its vertices unchanged.  Only integer atomics decide anything: the same bits from
    run to run, for any batch, stream, face order and table_slots (the edge table's size as in mesh_topology).  Scratch comes from the
    scratch cache ("mesh smooth").

    ValueError for wrong dtypes, shapes or devices, counts that are negative or do not sum to the packed lengths, a bad iters, lam, mu or
    table_slots -- all before any launch -- and, checked on the device and raised after the launches, for a vertex that is not finite and
    for a face index outside its image's vertex range (never dereferenced).

    Host synchronisation: one read of the two flags after the launches.  Runs on the current stream."""
    who = "shapeclipper_amd: mesh_smooth"
    B, V, F, _, offsets = check_packed(who, verts, faces, v_count, f_count, max_images=MESH_TOPOLOGY_MAX_IMAGES,
                                       max_faces=MESH_TOPOLOGY_MAX_FACES)
    dev = verts.device
    if V > MESH_SMOOTH_MAX_VERTS:
        raise ValueError("%s: verts: at most 2^30 vertices per call, got %d" % (who, V))
    if isinstance(iters, bool) or not isinstance(iters, int) or not 0 <= iters <= MESH_SMOOTH_MAX_ITERS:
        raise ValueError("%s: iters must be an integer in 0..%d, got %r" % (who, MESH_SMOOTH_MAX_ITERS, iters))
    if not _finite_number(lam) or not 0 < lam <= 1:
        raise ValueError("%s: lam must be a finite number in (0, 1], got %r" % (who, lam))
    if not _finite_number(mu) or not -1 <= mu <= 0:
        raise ValueError("%s: mu must be a finite number in [-1, 0], got %r" % (who, mu))
    table_slots = _edge_table_slots(who, F, table_slots)
    verts_out = torch.empty(V, 3, device=dev, dtype=torch.float32)
    counts = torch.zeros(len(MESH_SMOOTH_COUNTS), B, device=dev, dtype=torch.int64)
    measures = torch.zeros(len(MESH_SMOOTH_MEASURES), B, device=dev, dtype=torch.float64)
    if B > 0:
        offsets = offsets.to(dev)
        bad = torch.empty(2, device=dev, dtype=torch.int32)             # bad_vertex, bad_index
        lib = _lib.load()
        with torch.cuda.device(dev):
            ws = _scratch("mesh smooth", dev, (lib.sc_mesh_smooth_scratch_bytes(B, V, F, table_slots) + 3) // 4)
            code = lib.sc_mesh_smooth(_lib.ptr(verts.contiguous()) if V else None, _lib.ptr(faces.contiguous()) if F else None,
                                      _lib.ptr(offsets[0]), _lib.ptr(offsets[1]), B, V, F, table_slots, iters, float(lam), float(mu),
                                      _lib.ptr(ws), _lib.ptr(verts_out) if V else None, _lib.ptr(counts), _lib.ptr(measures),
                                      _lib.ptr(bad[:1]), _lib.ptr(bad[1:]), _lib.stream())
        _lib.check(code, "sc_mesh_smooth")
        flags = bad.tolist()
        if flags[0]:
            raise ValueError("%s: a vertex is not finite" % who)
        if flags[1]:
            raise ValueError("%s: a face index lies outside its image's vertex range [0, v_count[b])" % who)
    return SmoothedMesh(verts_out, faces, v_count, f_count, *counts.unbind(0), measures[2], measures[3], measures[0], measures[1])


# ---- post-processing: Loop subdivision of indexed triangle meshes and a Newton step onto the SDF's zero set (csrc/mesh_subdivide.hip) ----
MESH_SUBDIVIDE_MAX_LEVELS = 3
MESH_SUBDIVIDE_MAX_FACES = 1 << 24          # 4 F <= 2^26 per level
MESH_SUBDIVIDE_COUNTS = ("vertices_out", "edges", "sharp_edges", "fixed_vertices", "isolated", "degree_max")    # rows of sc_mesh_subdivide's counts


class SubdividedMesh(collections.namedtuple("SubdividedMesh", ("verts", "faces", "v_count", "f_count", "fixed", "edges", "sharp_edges",
                                                               "fixed_vertices"))):
    __slots__ = ()
    packed = property(lambda self: PackedMesh(*self[:4]), doc="the subdivided meshes alone, as a PackedMesh")


def mesh_subdivide(verts, faces, v_count, f_count, levels=1, table_slots=None):
    """Refines a PackedMesh (mesh_pack.py) of B images, passed as `*mesh` -- verts and faces on the device, v_count / f_count [B] int64 or
    int32 (host or device) -- by `levels` (1..3) steps of Loop subdivision with Warren's weights: every face becomes four, every edge gets
    a vertex, an old vertex keeps its number and moves to 0.625 x_i + (0.375 / n) sum of its n neighbours (0.4375 and 0.1875 at n = 3), the
    vertex of an edge with two faces is 3/8 of its ends plus 1/8 of the two opposite vertices.  An edge with one face (the open rim) or with
    three or more is sharp: its ends keep their bits, its new vertex is the midpoint, and all three are `fixed`; a vertex on no edge keeps
    its bits.  Float64 from the exactly widened input, every operation rounded once, the sums in ascending neighbour number; each level's
    output is rounded to fp32 once and is the next level's input.  include/shapeclipper_hip.h states every rule (sc_mesh_subdivide);
    tests/mesh_subdivide_ref.py restates them in numpy.

    -> SubdividedMesh(verts [V',3] fp32, faces [4^levels F,3] int32 image-local, v_count, f_count [B] int64 on the host -- `.packed` is
    these four as a PackedMesh again --, fixed [V'] bool on the device, edges, sharp_edges, fixed_vertices [B] int64 on the device, of the
    last level's input).  Image b's vertices are [old | new], a new vertex numbered by its edge's first half-edge in face order; face f
    becomes faces 4 f .. 4 f + 3 with the winding kept.  Only integer atomics decide anything: the same bits from run to run, for any
    batch, stream and table_slots (the edge table's size as in mesh_topology; it is used for a level whose 3 F it exceeds, else the
    default).  Scratch comes from the scratch cache ("mesh subdivide").

    ValueError for wrong dtypes, shapes or devices, counts that are negative or do not sum to the packed lengths, a bad levels or
    table_slots, more than 2^24 faces going into a level -- all before any launch -- and, checked on the device and raised after a level's
    launches, for a vertex that is not finite, a face index outside its image's vertex range (never dereferenced) and a face that repeats
    an index.

    Host synchronisation: one read per level, of the per-image counts that size the outputs and of the three flags.  Runs on the current
    stream."""
    who = "shapeclipper_amd: mesh_subdivide"
    B, V, F, counts_host, offsets = check_packed(who, verts, faces, v_count, f_count, max_images=MESH_TOPOLOGY_MAX_IMAGES,
                                                 max_faces=MESH_TOPOLOGY_MAX_FACES)
    dev = verts.device
    if V > MESH_SMOOTH_MAX_VERTS:
        raise ValueError("%s: verts: at most 2^30 vertices per call, got %d" % (who, V))
    if isinstance(levels, bool) or not isinstance(levels, int) or not 1 <= levels <= MESH_SUBDIVIDE_MAX_LEVELS:
        raise ValueError("%s: levels must be an integer in 1..%d, got %r" % (who, MESH_SUBDIVIDE_MAX_LEVELS, levels))
    if F * 4 ** (levels - 1) > MESH_SUBDIVIDE_MAX_FACES:
        raise ValueError("%s: faces: at most 2^24 faces may go into a level (4 F <= 2^26), got %d into level %d" % (who, F * 4 ** (levels - 1), levels))
    table_slots = _edge_table_slots(who, F, table_slots, default=False)
    fixed = torch.zeros(V, device=dev, dtype=torch.bool)
    n_fields = len(MESH_SUBDIVIDE_COUNTS)
    counts = torch.zeros(n_fields, B, device=dev, dtype=torch.int64)
    if B == 0:
        return SubdividedMesh(verts, faces, counts_host[0], counts_host[1], fixed, counts[1], counts[2], counts[3])
    lib = _lib.load()
    verts, faces = verts.contiguous(), faces.contiguous()
    for level in range(levels):
        slots = table_slots if table_slots is not None and table_slots > 3 * F else mesh_topology_slots(F)
        verts_out = torch.empty(V + 3 * F, 3, device=dev, dtype=torch.float32)
        faces_out = torch.empty(4 * F, 3, device=dev, dtype=torch.int32)
        fixed = torch.empty(V + 3 * F, device=dev, dtype=torch.bool)
        back = torch.zeros(n_fields * B + 2, device=dev, dtype=torch.int64)         # what the host reads: the counts, then the three flags
        counts, bad = back[:n_fields * B].view(n_fields, B), back[n_fields * B:].view(torch.int32)     # bad_vertex, bad_index, bad_face
        offsets = offsets.to(dev)
        with torch.cuda.device(dev):
            ws = _scratch("mesh subdivide", dev, (lib.sc_mesh_subdivide_scratch_bytes(B, V, F, slots) + 3) // 4)
            code = lib.sc_mesh_subdivide(_lib.ptr(verts) if V else None, _lib.ptr(faces) if F else None, _lib.ptr(offsets[0]),
                                         _lib.ptr(offsets[1]), B, V, F, slots, _lib.ptr(ws), _lib.ptr(verts_out) if V + F else None,
                                         _lib.ptr(faces_out) if F else None, _lib.ptr(fixed) if V + F else None, _lib.ptr(counts),
                                         _lib.ptr(bad[:1]), _lib.ptr(bad[1:2]), _lib.ptr(bad[2:3]), _lib.stream())
        _lib.check(code, "sc_mesh_subdivide")
        host = back.cpu()
        flags = host[n_fields * B:].view(torch.int32).tolist()
        if flags[0]:
            raise ValueError("%s: a vertex is not finite" % who)
        if flags[1]:
            raise ValueError("%s: a face index lies outside its image's vertex range [0, v_count[b])" % who)
        if flags[2]:
            raise ValueError("%s: a face repeats a vertex index" % who)
        counts_host = torch.stack([host[:B], 4 * counts_host[1]])
        V, F = int(counts_host[0].sum()), 4 * F
        verts, faces, fixed = verts_out[:V], faces_out, fixed[:V]
        offsets = PackedMesh(verts, faces, counts_host[0], counts_host[1]).offsets()
    return SubdividedMesh(verts, faces, counts_host[0], counts_host[1], fixed, counts[1], counts[2], counts[3])


def mesh_project_step(verts, sdf, grad, fixed, scale, max_step):
    """One clamped Newton step of vertices onto the zero set of an SDF: verts [V,3] fp32, sdf [V] and grad [V,3] fp32 (the value and d sdf /
    d position at the vertices, in the SDF's own units), fixed [V] bool, all on one device -> verts' [V,3] fp32,
    v' = v - d, d = scale sdf grad / |grad|^2, shortened to `max_step` where it is longer.  `scale` (> 0) turns the SDF's units into those
    of verts, `max_step` (>= 0) is in the units of verts.  A vertex keeps its bits if it is fixed, if sdf or |grad|^2 is not finite or
    |grad|^2 < 1e-12, or if the step's length is not finite.  Elementwise fp32, every operation rounded once (sc_mesh_project_step in
    include/shapeclipper_hip.h; tests/mesh_subdivide_ref.py restates it in numpy).  ValueError for wrong dtypes, shapes, devices or
    numbers, before any launch.  No host synchronisation; runs on the current stream."""
    who = "mesh_project_step"
    verts = device_tensor(who, "verts", verts, (torch.float32,))
    dev = verts.device
    sdf = device_tensor(who, "sdf", sdf, (torch.float32,), dev)
    grad = device_tensor(who, "grad", grad, (torch.float32,), dev)
    fixed = device_tensor(who, "fixed", fixed, (torch.bool,), dev)
    V = verts.shape[0]
    if verts.dim() != 2 or verts.shape[1] != 3 or grad.shape != verts.shape or sdf.shape != (V,) or fixed.shape != (V,):
        raise ValueError("shapeclipper_amd: %s takes verts [V,3], sdf [V], grad [V,3] and fixed [V], got %s, %s, %s and %s"
                         % (who, tuple(verts.shape), tuple(sdf.shape), tuple(grad.shape), tuple(fixed.shape)))
    if V > MESH_SMOOTH_MAX_VERTS:
        raise ValueError("shapeclipper_amd: %s: verts: at most 2^30 vertices per call, got %d" % (who, V))
    if not _finite_number(scale) or not scale > 0:
        raise ValueError("shapeclipper_amd: %s: scale must be a finite number > 0, got %r" % (who, scale))
    if not _finite_number(max_step) or not max_step >= 0:
        raise ValueError("shapeclipper_amd: %s: max_step must be a finite number >= 0, got %r" % (who, max_step))
    out = torch.empty_like(verts)
    if V:
        lib = _lib.load()
        with torch.cuda.device(dev):
            code = lib.sc_mesh_project_step(_lib.ptr(verts), _lib.ptr(sdf), _lib.ptr(grad), _lib.ptr(fixed), V, float(scale), float(max_step),
                                            _lib.ptr(out), _lib.stream())
        _lib.check(code, "sc_mesh_project_step")
    return out


# ---- post-processing: quadric edge-collapse decimation of indexed triangle meshes to a face budget (csrc/mesh_decimate.hip) --------------
MESH_DECIMATE_TARGET = (4, 1 << 24)         # the face budget ops.mesh_decimate takes
MESH_DECIMATE_MAX_ROUNDS = 4096
MESH_DECIMATE_COUNTS = ("faces_out", "selected", "collapsed", "candidates", "rejected_link", "rejected_flip", "fixed_vertices")   # rows of a round's counts
MESH_DECIMATE_TALLIES = ("rounds", "collapses", "rejected_link", "rejected_flip", "fixed_vertices", "reached")


class DecimatedMesh(collections.namedtuple("DecimatedMesh", ("verts", "faces", "v_count", "f_count", "vertex_map", "fixed") + MESH_DECIMATE_TALLIES)):
    __slots__ = ()
    packed = property(lambda self: PackedMesh(*self[:4]), doc="the decimated meshes alone, as a PackedMesh")


def mesh_decimate(verts, faces, v_count, f_count, target_faces, reg=1e-3, max_rounds=1024, table_slots=None):
    """Decimates a PackedMesh (mesh_pack.py) of B images, passed as `*mesh` -- verts and faces on the device, v_count / f_count [B] int64 or
    int32 (host or device) -- to `target_faces` (4..2^24) faces per image by quadric edge collapses.  One ROUND (sc_mesh_decimate_round) is a
    pure function of the current mesh: vertex quadrics from the current faces; the candidate edges (two faces, not both ends fixed, the
    link condition, not the tetrahedron case); for each the minimiser of the summed quadric, regularised towards the midpoint by `reg`
    (in (0, 1]), or the fixed end's position, and its cost; candidates that would turn a face over are dropped; of the rest a
    deterministic independent set -- an edge goes iff its key (cost as fp32 bits, then its lowest half-edge) is the minimum over its
    closed neighbourhood --; at most ceil((F - target_faces) / 2) of them, the cheapest, collapse: the survivor (the fixed end, else the
    lower number) moves, two faces go.  Vertices on an edge with one face (the rim that the grid face cuts) or three and more are fixed:
    never moved, never removed.  Rounds repeat until every image is at or below target_faces, an image's round selects nothing (it is
    then left alone), or `max_rounds` (1..4096) are done; an image ends at target_faces or target_faces - 1 unless its candidates run out.
    Float64 from the exactly widened input, every operation rounded once, sums in ring order, positions rounded to fp32 once when written.
    include/shapeclipper_hip.h states every rule; tests/mesh_decimate_ref.py restates them in numpy.

    -> DecimatedMesh(verts [V',3] fp32, faces [F',3] int32 image-local, v_count, f_count [B] int64 on the host -- `.packed` is these four
    as a PackedMesh again --, vertex_map [V] int32 (the output vertex an input vertex ended in, -1 for one no face uses in the end), fixed
    [V'] bool (the vertex was fixed in the INPUT mesh), and per image, [B] int64 on the host: rounds, collapses, rejected_link and
    rejected_flip (sums over the image's rounds), fixed_vertices (of the input mesh), reached (1 iff f_count <= target_faces)).  The
    output vertices are those a face still uses, in ascending input number; the faces keep their order.  An image already at or below
    target_faces keeps every bit.  Only integer atomics decide anything: the same bits from run to run, for any batch, stream and
    table_slots (the edge table's size as in mesh_topology; by default sized for every round's face count).  Ties between equal costs
    break by half-edge number, so the result is NOT invariant under a permutation of the faces.  Scratch comes from the scratch cache
    ("mesh decimate").

    ValueError for wrong dtypes, shapes or devices, counts that are negative or do not sum to the packed lengths, a bad target_faces, reg,
    max_rounds or table_slots -- all before any launch -- and, checked on the device and raised after a round's launches, for a vertex
    that is not finite, a face index outside its image's vertex range (never dereferenced) and a face that repeats an index.

    Host synchronisation: one read per round, of the per-image counts and the three flags, and one of the output vertex counts.  Runs on
    the current stream."""
    who = "shapeclipper_amd: mesh_decimate"
    B, V, F, counts_host, offsets = check_packed(who, verts, faces, v_count, f_count, max_images=MESH_TOPOLOGY_MAX_IMAGES,
                                                 max_faces=MESH_TOPOLOGY_MAX_FACES)
    dev = verts.device
    if V > MESH_SMOOTH_MAX_VERTS:
        raise ValueError("%s: verts: at most 2^30 vertices per call, got %d" % (who, V))
    lo, hi = MESH_DECIMATE_TARGET
    if isinstance(target_faces, bool) or not isinstance(target_faces, int) or not lo <= target_faces <= hi:
        raise ValueError("%s: target_faces must be an integer in %d..%d, got %r" % (who, lo, hi, target_faces))
    if not _finite_number(reg) or not 0 < reg <= 1:
        raise ValueError("%s: reg must be a finite number in (0, 1], got %r" % (who, reg))
    if isinstance(max_rounds, bool) or not isinstance(max_rounds, int) or not 1 <= max_rounds <= MESH_DECIMATE_MAX_ROUNDS:
        raise ValueError("%s: max_rounds must be an integer in 1..%d, got %r" % (who, MESH_DECIMATE_MAX_ROUNDS, max_rounds))
    table_slots = _edge_table_slots(who, F, table_slots, default=False)
    tally = {k: torch.zeros(B, dtype=torch.int64) for k in MESH_DECIMATE_TALLIES}
    if B == 0:
        return DecimatedMesh(verts, faces, counts_host[0], counts_host[1], torch.zeros(V, device=dev, dtype=torch.int32),
                             torch.zeros(V, device=dev, dtype=torch.bool), *tally.values())
    lib = _lib.load()
    n_fields = len(MESH_DECIMATE_COUNTS)
    work, faces = verts.contiguous().clone(), faces.contiguous()        # a round moves its survivors in place
    parent = torch.arange(V, device=dev, dtype=torch.int32)
    fixed = torch.zeros(V, device=dev, dtype=torch.bool)
    f_count = counts_host[1].clone()
    offsets = offsets.to(dev)
    active = f_count > target_faces
    for n in range(max_rounds):
        slots = table_slots if table_slots is not None else mesh_topology_slots(F)
        faces_out = torch.empty(F, 3, device=dev, dtype=torch.int32)
        back = torch.zeros(n_fields * B + 2, device=dev, dtype=torch.int64)         # what the host reads: the counts, then the three flags
        counts, flags = back[:n_fields * B].view(n_fields, B), back[n_fields * B:].view(torch.int32)
        with torch.cuda.device(dev):
            ws = _scratch("mesh decimate", dev, (lib.sc_mesh_decimate_scratch_bytes(B, V, F, slots) + 3) // 4)
            code = lib.sc_mesh_decimate_round(_lib.ptr(work) if V else None, _lib.ptr(faces) if F else None, _lib.ptr(offsets[0]),
                                              _lib.ptr(offsets[1]), B, V, F, slots, target_faces, float(reg), _lib.ptr(ws),
                                              _lib.ptr(parent) if V else None, _lib.ptr(faces_out) if F else None,
                                              _lib.ptr(fixed) if V and n == 0 else None, _lib.ptr(counts), _lib.ptr(flags), _lib.stream())
        _lib.check(code, "sc_mesh_decimate_round")
        host = back.cpu()
        bad = host[n_fields * B:].view(torch.int32).tolist()
        if bad[0]:
            raise ValueError("%s: a vertex is not finite" % who)
        if bad[1]:
            raise ValueError("%s: a face index lies outside its image's vertex range [0, v_count[b])" % who)
        if bad[2]:
            raise ValueError("%s: a face repeats a vertex index" % who)
        c = dict(zip(MESH_DECIMATE_COUNTS, host[:n_fields * B].view(n_fields, B)))
        if n == 0:
            tally["fixed_vertices"] = c["fixed_vertices"].clone()
        took_part = active.long()
        tally["rounds"] += took_part
        tally["collapses"] += took_part * c["collapsed"]
        tally["rejected_link"] += took_part * c["rejected_link"]
        tally["rejected_flip"] += took_part * c["rejected_flip"]
        f_count = c["faces_out"].clone()
        F = int(f_count.sum())
        faces = faces_out[:F]
        offsets = torch.stack([offsets[0], torch.cat([torch.zeros(1, dtype=torch.int64), f_count.cumsum(0)]).to(dev)])
        active = active & (c["selected"] > 0) & (f_count > target_faces)            # an image whose round selects nothing is left alone
        if not bool(active.any()):
            break
    tally["reached"] = (f_count <= target_faces).long()
    verts_out = torch.empty(V, 3, device=dev, dtype=torch.float32)
    faces_final = torch.empty(F, 3, device=dev, dtype=torch.int32)
    vertex_map = torch.empty(V, device=dev, dtype=torch.int32)
    fixed_out = torch.empty(V, device=dev, dtype=torch.bool)
    v_count_out = torch.zeros(B, device=dev, dtype=torch.int64)
    with torch.cuda.device(dev):
        ws = _scratch("mesh decimate", dev, (lib.sc_mesh_decimate_scratch_bytes(B, V, F, mesh_topology_slots(F)) + 3) // 4)
        code = lib.sc_mesh_decimate_compact(_lib.ptr(work) if V else None, _lib.ptr(faces) if F else None, _lib.ptr(offsets[0]),
                                            _lib.ptr(offsets[1]), B, V, F, _lib.ptr(parent) if V else None, _lib.ptr(fixed) if V else None,
                                            _lib.ptr(ws), _lib.ptr(verts_out) if V else None, _lib.ptr(faces_final) if F else None,
                                            _lib.ptr(vertex_map) if V else None, _lib.ptr(fixed_out) if V else None, _lib.ptr(v_count_out),
                                            _lib.stream())
    _lib.check(code, "sc_mesh_decimate_compact")
    v_out = v_count_out.cpu()
    n_out = int(v_out.sum())
    return DecimatedMesh(verts_out[:n_out], faces_final, v_out, f_count, vertex_map, fixed_out[:n_out], *(tally[k] for k in MESH_DECIMATE_TALLIES))


# ---- shading: ambient occlusion of surface points from the dense level grid (csrc/level_ao.hip) ------------------------------------------
LEVEL_AO_DIRS = 64                          # SC_LEVEL_AO_DIRS: one direction per lane of a wave
LEVEL_AO_MAX_STEPS = 4096                   # SC_LEVEL_AO_MAX_STEPS
LEVEL_AO_MAX_AXIS = 1024
LEVEL_AO_MAX_IMAGES = 65535
LEVEL_AO_MAX_POINTS = 1 << 30
AmbientOcclusion = collections.namedtuple("AmbientOcclusion", ["ao", "mask"])
_AO_DIRS = {}                               # device index -> ao_directions() on that device


def ao_directions():
    """The 64 directions of level_ambient_occlusion, [64,3] numpy float32: the Fibonacci set z = 1 - (2 k + 1) / 64, r = sqrt(1 - z^2),
    phi = k pi (3 - sqrt 5), (r cos phi, r sin phi, z), computed in float64 and rounded once.  They are data to the kernel, which
    evaluates no sine; a direction and its opposite serve as one, since every direction is folded into the normal's hemisphere."""
    k = np.arange(LEVEL_AO_DIRS, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / LEVEL_AO_DIRS
    r = np.sqrt(1.0 - z * z)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(np.float32)


def ao_step_count(radius, step):
    """M = ceil(radius / step), the samples per ray of level_ambient_occlusion, in host float64; ValueError unless radius and step are
    finite numbers > 0 and M lies in 1..4096."""
    who = "shapeclipper_amd: level_ambient_occlusion"
    for name, x in (("radius", radius), ("step", step)):
        if not _finite_number(x) or not x > 0:
            raise ValueError("%s: %s must be a finite number > 0, got %r" % (who, name, x))
    M = int(math.ceil(radius / step))
    if not 1 <= M <= LEVEL_AO_MAX_STEPS:
        raise ValueError("%s: radius / step = %r / %r asks for %d samples per ray; 1..%d are possible" % (who, radius, step, M, LEVEL_AO_MAX_STEPS))
    return M


def level_ambient_occlusion(level, points, normals, image, radius, step=0.5, bias=1.0, iso=0.0, cell_skip=True):
    """Ambient occlusion of N surface points from the dense level grid: level [B,S,S,S] fp32 (index (x S + y) S + z, 2 <= S <= 1024),
    points [N,3] fp32 in grid-index units (the units of isosurface_mesh's vertices), normals [N,3] fp32 of any length, image [N] int32,
    all on one device -> AmbientOcclusion(ao [N] fp32 in [0, 1], mask [N] int64).  From every point 64 rays (ao_directions, each folded
    into the normal's hemisphere) start at p + bias n and take M = ceil(radius / step) samples `step` grid pitches apart (radius in grid
    pitches); a ray is closed by the first sample whose trilinear level is < iso and open when it leaves the grid or ends.  ao is the
    |D . n|-weighted share of the open rays -- 1 on a convex shape, 0.5 in a right-angled crease, towards 0 in a pit -- and bit k of
    mask says direction k is open.  A point or normal that is not finite and a zero normal give ao = 1 and mask = -1.
    include/shapeclipper_hip.h states every operation (sc_level_ambient_occlusion); tests/level_ao_ref.py restates them in numpy.

    cell_skip=True: a first launch writes the bit volume of the cells with a corner < iso and the march tests a sample's bit before it
    loads 8 floats; False: the corner test comes from the loads.  The same bits either way, from run to run, for any batch, stream and
    order of the points: there are no atomics.  The bit volume comes from the scratch cache ("level ao").

    ValueError for wrong dtypes, shapes or devices, a bad number, radius / step outside 1..4096 samples -- all before any launch -- and,
    flagged on the device (never dereferenced) and raised after the launches, for an image outside 0..B-1.  N = 0 returns empty tensors
    without a launch.  Host synchronisation: one read of the flag.  Runs on the current stream."""
    who = "level_ambient_occlusion"
    level = device_tensor(who, "level", level, (torch.float32,))
    dev = level.device
    points = device_tensor(who, "points", points, (torch.float32,), dev)
    normals = device_tensor(who, "normals", normals, (torch.float32,), dev)
    image = device_tensor(who, "image", image, (torch.int32,), dev)
    if level.dim() != 4 or not (level.shape[1] == level.shape[2] == level.shape[3]) or not 2 <= level.shape[1] <= LEVEL_AO_MAX_AXIS \
            or not 1 <= level.shape[0] <= LEVEL_AO_MAX_IMAGES:
        raise ValueError("shapeclipper_amd: %s takes level [B,S,S,S] with 1 <= B <= %d and 2 <= S <= %d, got %s"
                         % (who, LEVEL_AO_MAX_IMAGES, LEVEL_AO_MAX_AXIS, tuple(level.shape)))
    B, S, N = level.shape[0], level.shape[1], points.shape[0]
    if points.dim() != 2 or points.shape[1] != 3 or normals.shape != points.shape or tuple(image.shape) != (N,) or N > LEVEL_AO_MAX_POINTS:
        raise ValueError("shapeclipper_amd: %s takes points [N,3], normals [N,3] and image [N] with N <= 2^30, got %s, %s and %s"
                         % (who, tuple(points.shape), tuple(normals.shape), tuple(image.shape)))
    M = ao_step_count(radius, step)
    for name, x in (("bias", bias), ("iso", iso)):
        if not _finite_number(x):
            raise ValueError("shapeclipper_amd: %s: %s must be a finite number, got %r" % (who, name, x))
    if not isinstance(cell_skip, bool):
        raise ValueError("shapeclipper_amd: %s: cell_skip must be a bool, got %r" % (who, cell_skip))
    ao = torch.empty(N, device=dev, dtype=torch.float32)
    mask = torch.empty(N, device=dev, dtype=torch.int64)
    if N == 0:
        return AmbientOcclusion(ao, mask)
    dirs = _AO_DIRS.get(dev.index)
    if dirs is None:
        dirs = _AO_DIRS[dev.index] = torch.from_numpy(ao_directions()).to(dev)
    bad = torch.empty(1, device=dev, dtype=torch.int32)
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = _scratch("level ao", dev, (lib.sc_level_ao_scratch_bytes(B, S) + 3) // 4) if cell_skip else None
        code = lib.sc_level_ambient_occlusion(_lib.ptr(level), _lib.ptr(points), _lib.ptr(normals), _lib.ptr(image), _lib.ptr(dirs), B, S, N,
                                              float(step), float(bias), float(iso), M, 1 if cell_skip else 0, _lib.ptr(ws), _lib.ptr(ao),
                                              _lib.ptr(mask), _lib.ptr(bad), _lib.stream())
    _lib.check(code, "sc_level_ambient_occlusion")
    if bad.tolist()[0]:
        raise ValueError("shapeclipper_amd: %s: an image index lies outside 0..B-1 = 0..%d" % (who, B - 1))
    return AmbientOcclusion(ao, mask)
