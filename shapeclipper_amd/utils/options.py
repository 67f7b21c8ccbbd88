"""YAML + `--a.b.c=value` command-line configuration, same semantics as the reference's
utils/options.py (parse_arguments :16-34, set :36-44, _parent_ inheritance :46-60, process_options
:79-95) with two deliberate differences for unattended runs: an unknown CLI key and a changed
options.yaml never block on input() unless stdin is a TTY (benchmarks / CI must not hang)."""
from __future__ import annotations

import collections
import importlib
import os
import random
import string
import sys

import numpy as np
import torch
import yaml

from . import util
from .util import EasyDict as edict
from .util import log

torch.backends.cudnn.benchmark = False

# The `hip.*` switches of this build, one row each: (key, default, kind, what it selects, the (module, attribute) it drives | None).
# kind is bool, or (lo, hi) for an integer in lo..hi (hi None: no upper bound here).  A reference YAML without these keys still loads:
# `set` fills in the defaults, and `hip(opt, key)` answers with them for an option tree that has no `hip` node.  Modules are named
# relative to the package; process_options writes bool(value) into every attribute named here.
Switch = collections.namedtuple("Switch", ["key", "default", "kind", "text", "drives"])
HIP_TABLE = tuple(Switch(*row) for row in (
    ("device_rng", False, bool, "draw the render's jitter on the GPU (no 4 MB upload per render, another random stream than the reference)", None),
    ("device_choice", True, bool, "pick the regularisation view on the device (reg.n_views = 1)", None),
    ("device_rays", True, bool, "Pix3D: silhouette-weighted ray choice for the whole batch on the GPU (csrc/silhouette_rays.hip)", None),
    ("device_clip_preprocess", True, bool, "Pix3D: CLIP preprocessing on the GPU (csrc/clip_preprocess.hip)", None),
    ("fused_backward", True, bool, "SDF reverse pass with the weight gradients formed in the kernel (sc_sdf_backward_fused)", None),
    # the reference sets cudnn.deterministic=True globally (utils/options.py:14); on ROCm that restricts MIOpen to GEMM-based backward
    # solvers (measured 437 ms of 640 ms per bs32 step), so it is opt-in here
    ("deterministic_conv", False, bool, "torch.backends.cudnn.deterministic, process-global", None),
    ("fused_loss", True, bool, "the render losses of one render in a single launch (csrc/loss.hip)", None),
    ("fused_adam", True, bool, "torch's fused Adam on the device", None),
    ("guarded_step", True, bool, "a non-finite loss skips the update on the device; the host raises one step later", None),
    ("batched_encoders", True, bool, "one grouped encoder pass and one grouped estimator pass per step", None),
    ("two_streams", True, bool, "the view estimator runs on a side stream next to the encoders", None),
    ("overlap_allreduce", False, bool, "multi-GPU: the early gradient segment is all-reduced from inside backward", None),
    ("reserve_cus", 0, (0, None), "multi-GPU: persistent convolution grids sized for the device's CUs minus this many", None),
    ("fused_block", True, bool, "one autograd node per stride-1 BasicBlock", ("model.resnet", "FUSED_BLOCK")),
    ("fused_bottleneck", True, bool, "1x1 Bottleneck_Linear blocks as fused launches (csrc/bottleneck.hip)", ("model.view_estimator", "HIP_BOTTLENECK")),
    ("fused_rgb_wgrad", True, bool, "RGB reverse pass forms the weight gradients in the kernel; off: Gy_l / r_l through HBM and sc_wgrad",
     ("ops", "FUSED_RGB_WGRAD")),
    ("rgb_stash", True, bool, "RGB forward parks its hidden activations for the reverse pass; off: the reverse pass recomputes them",
     ("ops", "RGB_STASH")),
    ("value_split", True, bool, "value-only SDF calls (evaluation grid) on the pre-split bf16x3 chain; off: fp32 MFMA", ("ops", "SDF_VALUE_SPLIT")),
    ("rgb_split", True, bool, "RGB network of the forward pass from pre-split bf16x3 fragments; off: fp32 MFMA", ("ops", "RGB_FWD_SPLIT")),
    ("rgb_bwd_split", True, bool, "RGB reverse chain from pre-split transposed fragments; off: fp32 MFMA (see HIP_REQUIRES)",
     ("ops", "RGB_BWD_SPLIT")),
    ("sdf_stream", True, bool, "SDF forward (value, feature, d sdf/dx) from streamed pre-split fragments; off: fp32 MFMA", ("ops", "SDF_FWD_STREAM")),
    ("upload_stream", True, bool, "the CPU-generator draws are copied on a stream of their own, ahead of the render",
     ("model.renderer", "UPLOAD_STREAM")),
    # (the bottleneck blocks and the per-image latent biases no longer go through a BLAS at all -- csrc/bottleneck.hip, latent_bias.hip --
    # so what this switch still touches are the ~20 remaining small products of a step: final projector / head Linears.)  rocBLAS instead
    # of torch's default hipBLASLt: 7 instead of 18 us of host time per call (a host-paced B=8 step 16.3 -> 14.9 ms)
    ("rocblas", True, bool, "the small fp32 GEMMs left to torch go through rocBLAS, process-global; off leaves torch's choice alone", None),
    ("conv3x3", True, bool, "3x3 stride-1 trunk convolutions on csrc/conv3x3.hip", ("model.resnet", "HIP_CONV3X3")),
    ("conv3x3_split", True, bool, "... as exact three-piece bf16 operand splits; off: fp32 MFMA throughout", ("model.resnet", "HIP_CONV3X3_SPLIT")),
    ("conv_stem", True, bool, "the 7x7 stride-2 stem convolution on its HIP kernel", ("model.resnet", "HIP_CONV_STEM")),
    ("conv1x1", True, bool, "the 1x1 stride-2 shortcut convolutions on their HIP kernels", ("model.resnet", "HIP_CONV_1X1")),
    ("conv3x3s2", True, bool, "the 3x3 stride-2 convolutions' forward on its HIP kernel", ("model.resnet", "HIP_CONV3X3_S2")),
    ("conv3x3s2_grads", True, bool, "... and their backward-data / weight gradient", ("model.resnet", "HIP_CONV3X3_S2_GRADS")),
    ("train_vis", False, bool, "training-time visualisation on rank 0: turn-table GIFs and periodic dumps", None),
    ("mesh_color", False, bool, "every mesh dump also writes a coloured PLY with vertex normals", None),
    ("largest_component", False, bool, "evaluation keeps the largest connected component of the level grid", None),
    ("surface_render", False, bool, "every per-sample dump also gets a render at the SDF zero crossing (Renderer.render_surface)", None),
    ("surface_refine", 3, (0, 16), "... refinement rounds of the crossing", None),
    ("surface_scale", 1, (1, 4), "... pixels per pixel side", None),
))
HIP = {row.key: row for row in HIP_TABLE}
# a switch that only counts while others are on: the split reverse chain is a form of the fused kernel that reads the parked activations
HIP_REQUIRES = {"rgb_bwd_split": ("rgb_stash", "fused_rgb_wgrad")}
HIP_DEFAULTS = dict(hip={row.key: row.default for row in HIP_TABLE})
_PACKAGE = __name__.rsplit(".", 2)[0]


def hip(opt, key):
    """opt.hip[key] where the option tree has it, else the table's default (trees built by hand need no `hip` node).  A key the table
    does not have is a KeyError: a mistake at the call site, not user input."""
    default = HIP[key].default
    return opt.get("hip", {}).get(key, default)


def dual_mesh_reg(opt):
    """The evaluation's dual-contouring dump: None unless `--eval.dual_mesh` is set (absent means off), else `--eval.dual_reg` (default
    0.05), the weight that holds a cell's vertex near the mean of its crossings (ops.dual_contour_mesh).  An evaluation setting beside
    eval.vox_res, not a hip.* switch.  A dual_reg that is not a real number in (0, 1] is a ValueError, whether or not the dump is on."""
    ev = opt.get("eval", None) or {}
    reg = ev.get("dual_reg", 0.05)
    if isinstance(reg, bool) or not isinstance(reg, (int, float)) or not 0.0 < reg <= 1.0:
        raise ValueError("eval.dual_reg must be a float in (0, 1], got %r" % (reg,))
    return float(reg) if ev.get("dual_mesh", False) else None


def texture_texels(opt, always=False):
    """The evaluation's textured OBJ dump: None unless `--eval.texture` is set (absent means off), else `--eval.texture_texels` (default
    8, an integer in 4..32), the side T in texels of the square atlas cell that two faces share (eval_3D.mesh_texture;
    include/shapeclipper_hip.h states the layout).  Evaluation settings beside eval.vox_res, not hip.* switches.  A bad value is a
    ValueError, whether or not the switch is on.  always=True returns T whatever the switch says (a direct call of mesh_texture)."""
    ev = opt.get("eval", None) or {}
    on, texels = ev.get("texture", False), ev.get("texture_texels", 8)
    if not isinstance(on, bool):
        raise ValueError("eval.texture must be a bool, got %r" % (on,))
    if isinstance(texels, bool) or not isinstance(texels, int) or not 4 <= texels <= 32:
        raise ValueError("eval.texture_texels must be an integer in 4..32, got %r" % (texels,))
    return texels if on or always else None


def mesh_render(opt):
    """The evaluation's picture of the textured mesh and its mask IoU (eval_3D.mesh_render, mesh_render.txt): `--eval.mesh_render`, absent
    means off.  An evaluation setting beside eval.texture, not a hip.* switch; it bakes the texture (eval.texture_texels) when
    `--eval.texture` has not.  A value that is not a bool is a ValueError, whether or not the switch is on."""
    on = (opt.get("eval", None) or {}).get("mesh_render", False)
    if not isinstance(on, bool):
        raise ValueError("eval.mesh_render must be a bool, got %r" % (on,))
    return on


def icp_settings(opt):
    """The evaluation's ICP-aligned metrics: None unless `--eval.icp` is set (absent means off), else (iters, scale) from
    `--eval.icp_iters` (default 30, an integer in 1..100) and `--eval.icp_scale` (default true: fit a similarity; false: a rigid motion),
    the arguments of ops.icp_align.  Evaluation settings beside eval.vox_res, not hip.* switches.  A bad value is a ValueError, whether
    or not the switch is on."""
    ev = opt.get("eval", None) or {}
    on, iters, scale = ev.get("icp", False), ev.get("icp_iters", 30), ev.get("icp_scale", True)
    if not isinstance(on, bool):
        raise ValueError("eval.icp must be a bool, got %r" % (on,))
    if isinstance(iters, bool) or not isinstance(iters, int) or not 1 <= iters <= 100:
        raise ValueError("eval.icp_iters must be an integer in 1..100, got %r" % (iters,))
    if not isinstance(scale, bool):
        raise ValueError("eval.icp_scale must be a bool, got %r" % (scale,))
    return (iters, scale) if on else None


def normal_settings(opt):
    """The evaluation's normal consistency: None unless `--eval.normals` is set (absent means off), else `--eval.normals_k` (default 16,
    an integer in 3..32), the neighbour count of ops.point_normals for the ground truth's PCA normals.  Evaluation settings beside
    eval.vox_res, not hip.* switches.  A bad value is a ValueError, whether or not the switch is on."""
    ev = opt.get("eval", None) or {}
    on, k = ev.get("normals", False), ev.get("normals_k", 16)
    if not isinstance(on, bool):
        raise ValueError("eval.normals must be a bool, got %r" % (on,))
    if isinstance(k, bool) or not isinstance(k, int) or not 3 <= k <= 32:
        raise ValueError("eval.normals_k must be an integer in 3..32, got %r" % (k,))
    return k if on else None


def mesh_dist_settings(opt):
    """The evaluation's mesh-based completeness: None unless `--eval.mesh_dist` is set (absent means off), else True -- the distance
    from every ground-truth point to the predicted MESH (eval_3D.mesh_metrics, ops.point_mesh_distance) beside the sample-based
    metrics.  An evaluation setting beside eval.vox_res, not a hip.* switch.  A value that is not a bool is a ValueError, whether or
    not the switch is on."""
    ev = opt.get("eval", None) or {}
    on = ev.get("mesh_dist", False)
    if not isinstance(on, bool):
        raise ValueError("eval.mesh_dist must be a bool, got %r" % (on,))
    return True if on else None


def emd_settings(opt):
    """The evaluation's Earth Mover's Distance: None unless `--eval.emd` is set (absent means off), else (points, eps) from
    `--eval.emd_points` (default 1024, the count of the Pix3D benchmark; an integer in 2..2048, the sizes ops.emd_match takes) and
    `--eval.emd_eps` (default 1e-4, a float in (0, 0.25]: the last epsilon of the auction, which starts at 0.25), the arguments of
    eval_3D.emd_metrics.  Evaluation settings beside eval.vox_res, not hip.* switches.  A bad value is a ValueError, whether or not the
    switch is on.  (`--eval.emd_eps=1e-4` arrives as the string "1e-4" -- YAML 1.1 reads a float only with a dot, "1.0e-4" -- so a
    string that float() reads is taken as that number.)"""
    ev = opt.get("eval", None) or {}
    on, points, eps = ev.get("emd", False), ev.get("emd_points", 1024), ev.get("emd_eps", 1e-4)
    if isinstance(eps, str):
        try:
            eps = float(eps)
        except ValueError:
            pass
    if not isinstance(on, bool):
        raise ValueError("eval.emd must be a bool, got %r" % (on,))
    if isinstance(points, bool) or not isinstance(points, int) or not 2 <= points <= 2048:
        raise ValueError("eval.emd_points must be an integer in 2..2048, got %r" % (points,))
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not 0.0 < eps <= 0.25:
        raise ValueError("eval.emd_eps must be a float in (0, 0.25], got %r" % (eps,))
    return (points, float(eps)) if on else None


def iou_settings(opt):
    """The evaluation's volumetric IoU: None unless `--eval.iou` is set (absent means off), else (res, close) from `--eval.iou_res`
    (default 32, Pix3D's resolution; an integer in 8..64, the grids ops.voxel_solid takes) and `--eval.iou_close` (default 1, an
    integer in 0..2: the dilations that close the voxel shell before it is filled), the arguments of eval_3D.iou_metrics.  Evaluation
    settings beside eval.vox_res, not hip.* switches.  A bad value is a ValueError, whether or not the switch is on."""
    ev = opt.get("eval", None) or {}
    on, res, close = ev.get("iou", False), ev.get("iou_res", 32), ev.get("iou_close", 1)
    if not isinstance(on, bool):
        raise ValueError("eval.iou must be a bool, got %r" % (on,))
    if isinstance(res, bool) or not isinstance(res, int) or not 8 <= res <= 64:
        raise ValueError("eval.iou_res must be an integer in 8..64, got %r" % (res,))
    if isinstance(close, bool) or not isinstance(close, int) or not 0 <= close <= 2:
        raise ValueError("eval.iou_close must be an integer in 0..2, got %r" % (close,))
    return (res, close) if on else None


def mesh_stats_settings(opt):
    """The evaluation's mesh statistics: True when `--eval.mesh_stats` is set (absent means off) -- eval_3D.mesh_stats then reports
    watertightness, manifoldness, orientation, components, genus, area and volume of the meshes that are written (ops.mesh_topology).
    An evaluation setting beside eval.vox_res, not a hip.* switch.  A value that is not a bool is a ValueError."""
    on = (opt.get("eval", None) or {}).get("mesh_stats", False)
    if not isinstance(on, bool):
        raise ValueError("eval.mesh_stats must be a bool, got %r" % (on,))
    return on


def simplify_settings(opt):
    """The evaluation's decimated mesh: None unless `--eval.simplify=k` is given (absent means off), else (k, reg): k, an integer in
    2..16, is the side of a cluster cell in grid pitches and reg, `--eval.simplify_reg` (default 0.05, a float in (0, 1]), the pull of a
    cluster's vertex towards the mean of its vertices -- the arguments of eval_3D.meshes_simplified (ops.mesh_cluster_simplify).
    Evaluation settings beside eval.vox_res, not hip.* switches.  A bool or any other bad value is a ValueError, whether or not the
    switch is on.  (A string that float() reads is taken as that number, as for eval.emd_eps.)"""
    ev = opt.get("eval", None) or {}
    k, reg = ev.get("simplify", None), ev.get("simplify_reg", 0.05)
    if isinstance(reg, str):
        try:
            reg = float(reg)
        except ValueError:
            pass
    if k is not None and (isinstance(k, bool) or not isinstance(k, int) or not 2 <= k <= 16):
        raise ValueError("eval.simplify must be an integer in 2..16, got %r" % (k,))
    if isinstance(reg, bool) or not isinstance(reg, (int, float)) or not 0.0 < reg <= 1.0:
        raise ValueError("eval.simplify_reg must be a float in (0, 1], got %r" % (reg,))
    return None if k is None else (k, float(reg))


def parse_arguments(args):
    """--key1.key2=value ; --flag (true) ; --flag! (false)"""
    opt_cmd = {}
    for arg in args:
        assert arg.startswith("--")
        if "=" not in arg[2:]:
            key_str, value = (arg[2:-1], "false") if arg[-1] == "!" else (arg[2:], "true")
        else:
            key_str, value = arg[2:].split("=", 1)
        keys = key_str.split(".")
        sub = opt_cmd
        for k in keys[:-1]:
            sub = sub.setdefault(k, {})
        assert keys[-1] not in sub, keys[-1]
        sub[keys[-1]] = yaml.safe_load(value)
    return edict(opt_cmd)


def load_options(fname):
    with open(fname) as f:
        opt = edict(yaml.safe_load(f))
    if "_parent_" in opt:
        parents = opt.pop("_parent_")
        parents = [parents] if isinstance(parents, str) else parents
        for parent in parents:
            opt = override_options(load_options(parent), opt, key_stack=[])
    print("loading {}...".format(fname))
    return opt


def _ask(question):
    if not sys.stdin or not sys.stdin.isatty():
        return "y"
    ans = None
    while ans not in ("y", "n"):
        ans = input(question)
    return ans


def override_options(opt, opt_over, key_stack=None, safe_check=False):
    for key, value in opt_over.items():
        if isinstance(value, dict):
            opt[key] = override_options(opt.get(key, edict()), value, key_stack=key_stack + [key], safe_check=safe_check)
        else:
            if safe_check and key not in opt:
                if _ask("\"{}\" not found in original opt, add? (y/n) ".format(".".join(key_stack + [key]))) == "n":
                    print("safe exiting...")
                    sys.exit()
            opt[key] = value
    return opt


def set(opt_cmd={}, verbose=True):
    if verbose:
        log.info("setting configurations...")
    opt = load_options(opt_cmd.yaml)
    opt = override_options(opt, opt_cmd, key_stack=[], safe_check=True)
    for k, v in HIP_DEFAULTS.items():
        cur = opt.get(k, edict())
        for kk, vv in v.items():
            cur.setdefault(kk, vv)
        opt[k] = edict(cur)
    process_options(opt)
    if verbose:
        log.options(opt)
    return opt


def process_options(opt):
    if opt.seed is not None:
        random.seed(opt.seed)
        np.random.seed(opt.seed)
        torch.manual_seed(opt.seed)
        if torch.cuda.is_available():
            torch.cuda.manual_seed_all(opt.seed)
    else:
        opt.name += "_{}".format("".join(random.choice(string.ascii_uppercase) for _ in range(4)))
    opt.output_path = "{0}/{1}/{2}".format(opt.output_root, opt.group, opt.name)
    os.makedirs(opt.output_path, exist_ok=True)
    assert isinstance(opt.gpu, int)
    opt.device = "cpu" if opt.cpu or not torch.cuda.is_available() else "cuda:{}".format(opt.gpu)
    opt.H, opt.W = opt.image_size
    if "data" in opt and "dataset" in opt.data and opt.data.dataset not in opt.data and "pix3d" in opt.data:
        opt.data[opt.data.dataset] = opt.data.pix3d      # e.g. --data.dataset=synthetic reuses the Pix3D camera ranges
    for row in HIP_TABLE:
        if row.kind is not bool and None not in row.kind:
            (lo, hi), v = row.kind, hip(opt, row.key)
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError("hip.%s must be an integer in %d..%d, got %r" % (row.key, lo, hi, v))
    dual_mesh_reg(opt)
    texture_texels(opt)
    mesh_render(opt)
    icp_settings(opt)
    normal_settings(opt)
    mesh_dist_settings(opt)
    emd_settings(opt)
    iou_settings(opt)
    mesh_stats_settings(opt)
    simplify_settings(opt)
    torch.backends.cudnn.deterministic = bool(hip(opt, "deterministic_conv"))
    for row in HIP_TABLE:
        if row.drives is not None:
            module, attr = row.drives
            on = all(bool(hip(opt, k)) for k in (row.key,) + HIP_REQUIRES.get(row.key, ()))
            setattr(importlib.import_module("%s.%s" % (_PACKAGE, module)), attr, on)
    if bool(hip(opt, "rocblas")) and torch.cuda.is_available():
        try:
            torch.backends.cuda.preferred_blas_library("cublas")
        except Exception:       # noqa: BLE001  (older torch: no such switch)
            pass


def save_options_file(opt):
    fname = "{}/options.yaml".format(opt.output_path)
    if os.path.isfile(fname):
        with open(fname) as f:
            old = yaml.safe_load(f)
        if util.to_dict(opt) != old:
            print("existing options file found (different from current one)...")
            if _ask("override? (y/n) ") == "n":
                print("safe exiting...")
                sys.exit()
        else:
            print("existing options file found (identical)")
    else:
        print("(creating new options file...)")
    with open(fname, "w") as f:
        yaml.safe_dump(util.to_dict(opt), f, default_flow_style=False, indent=4)
