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


# The `eval.*` settings of the optional evaluation outputs, one row each: (key, default, kind, what it sets[, flag]).  kind is bool, (lo, hi)
# with integer bounds for an integer in lo..hi, or (lo, hi) with float bounds for a real number in (lo, hi].  flag "absent": None (the key
# missing) is a value too and means off; flag "str": a string that float() reads counts as that number (`--eval.emd_eps=1e-4` arrives as
# the string "1e-4" -- YAML 1.1 reads a float only with a dot, "1.0e-4").  These are evaluation settings beside eval.vox_res, not hip.*
# switches; an absent key means its default, so a reference YAML loads unchanged.  eval_setting() is the one place a value is checked: a
# bad value is a ValueError whether or not the switch it belongs to is on, and process_options asks for every row.  The functions below
# it answer what each output needs: None (or False) while its switch is off, else the arguments of its metric function.
Setting = collections.namedtuple("Setting", ["key", "default", "kind", "text", "flag"], defaults=("",))
EVAL_TABLE = tuple(Setting(*row) for row in (
    ("texture", False, bool, "textured OBJ dump: {idx}_mesh_tex.obj / .mtl / .png and texture.txt (eval_3D.mesh_texture)"),
    ("texture_texels", 8, (4, 32), "... the side in texels of the square atlas cell that two faces share (include/shapeclipper_hip.h)"),
    ("mesh_render", False, bool, "pictures of the textured mesh and their mask IoU, mesh_render.txt; bakes the texture when eval.texture is off"),
    ("dual_mesh", False, bool, "dual-contouring dump {idx}_mesh_dual.ply (read by its truth value)"),
    ("dual_reg", 0.05, (0.0, 1.0), "... the weight that holds a cell's vertex near the mean of its crossings (ops.dual_contour_mesh)"),
    ("icp", False, bool, "ICP-aligned metrics beside the raw ones (ops.icp_align)"),
    ("icp_iters", 30, (1, 100), "... iterations"),
    ("icp_scale", True, bool, "... fit a similarity; false: a rigid motion"),
    ("normals", False, bool, "normal consistency (eval_3D.normal_metrics)"),
    ("normals_k", 16, (3, 32), "... the neighbour count of ops.point_normals for the ground truth's PCA normals"),
    ("mesh_dist", False, bool, "completeness from every ground-truth point to the predicted MESH (ops.point_mesh_distance)"),
    ("emd", False, bool, "Earth Mover's Distance (eval_3D.emd_metrics)"),
    ("emd_points", 1024, (2, 2048), "... points matched, the sizes ops.emd_match takes; 1024 is the Pix3D benchmark's count"),
    ("emd_eps", 1e-4, (0.0, 0.25), "... the last epsilon of the auction, which starts at 0.25", "str"),
    ("iou", False, bool, "volumetric IoU (eval_3D.iou_metrics)"),
    ("iou_res", 32, (8, 64), "... voxels per side, the grids ops.voxel_solid takes; 32 is Pix3D's resolution"),
    ("iou_close", 1, (0, 2), "... dilations that close the voxel shell before it is filled"),
    ("mesh_stats", False, bool, "watertightness, manifoldness, orientation, components, genus, area and volume of the written meshes (ops.mesh_topology)"),
    ("simplify", None, (2, 16), "decimated mesh {idx}_mesh_simplified.ply: the side of a cluster cell in grid pitches (ops.mesh_cluster_simplify)",
     "absent"),
    ("simplify_reg", 0.05, (0.0, 1.0), "... the pull of a cluster's vertex towards the mean of its vertices", "str"),
))
EVAL = {row.key: row for row in EVAL_TABLE}


def _checked(group, row, v):
    """v checked against a Setting row of the table of `group` ("eval", "mesh"): the value, as the row's kind; a ValueError that names
    group.key otherwise."""
    key = row.key
    if row.kind is bool:
        if not isinstance(v, bool):
            raise ValueError("%s.%s must be a bool, got %r" % (group, key, v))
        return v
    if v is None and row.flag == "absent":
        return None
    lo, hi = row.kind
    if isinstance(lo, int):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError("%s.%s must be an integer in %d..%d, got %r" % (group, key, lo, hi, v))
        return v
    if row.flag == "str" and isinstance(v, str):
        try:
            v = float(v)
        except ValueError:
            pass
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not lo < v <= hi:
        raise ValueError("%s.%s must be a float in (%g, %g], got %r" % (group, key, lo, hi, v))
    return float(v)


def eval_setting(opt, key):
    """opt.eval[key] checked against its row of EVAL_TABLE, the row's default where the option tree has no such key."""
    row = EVAL[key]
    return _checked("eval", row, (opt.get("eval", None) or {}).get(key, row.default))


def dual_mesh_reg(opt):
    """None unless `--eval.dual_mesh` is set, else eval.dual_reg."""
    reg = eval_setting(opt, "dual_reg")
    return reg if (opt.get("eval", None) or {}).get("dual_mesh", False) else None


def texture_texels(opt, always=False):
    """None unless `--eval.texture` is set, else eval.texture_texels; always=True returns it whatever the switch says (a direct call of
    eval_3D.mesh_texture)."""
    on, texels = eval_setting(opt, "texture"), eval_setting(opt, "texture_texels")
    return texels if on or always else None


def mesh_render(opt):
    """`--eval.mesh_render`, a bool."""
    return eval_setting(opt, "mesh_render")


def icp_settings(opt):
    """None unless `--eval.icp` is set, else (iters, scale), the arguments of ops.icp_align."""
    on, iters, scale = (eval_setting(opt, k) for k in ("icp", "icp_iters", "icp_scale"))
    return (iters, scale) if on else None


def normal_settings(opt):
    """None unless `--eval.normals` is set, else eval.normals_k."""
    on, k = eval_setting(opt, "normals"), eval_setting(opt, "normals_k")
    return k if on else None


def mesh_dist_settings(opt):
    """None unless `--eval.mesh_dist` is set, else True."""
    return True if eval_setting(opt, "mesh_dist") else None


def emd_settings(opt):
    """None unless `--eval.emd` is set, else (points, eps), the arguments of eval_3D.emd_metrics."""
    on, points, eps = (eval_setting(opt, k) for k in ("emd", "emd_points", "emd_eps"))
    return (points, eps) if on else None


def iou_settings(opt):
    """None unless `--eval.iou` is set, else (res, close), the arguments of eval_3D.iou_metrics."""
    on, res, close = (eval_setting(opt, k) for k in ("iou", "iou_res", "iou_close"))
    return (res, close) if on else None


def mesh_stats_settings(opt):
    """`--eval.mesh_stats`, a bool."""
    return eval_setting(opt, "mesh_stats")


def simplify_settings(opt):
    """None unless `--eval.simplify=k` is given, else (k, reg), the arguments of eval_3D.meshes_simplified."""
    k, reg = eval_setting(opt, "simplify"), eval_setting(opt, "simplify_reg")
    return None if k is None else (k, reg)


# The `mesh.*` settings: post-processing of the mesh that is written, one Setting row each as in EVAL_TABLE.  They are not eval.* settings:
# nothing here is measured against the ground truth and no report file or gather belongs to them -- a post-processed mesh is another file
# in the dump and a one-line sidecar beside it.  An absent key, or an absent `mesh` group, means the default, so a reference YAML loads
# unchanged and nothing is written into the option tree.
MESH_TABLE = tuple(Setting(*row) for row in (
    ("smooth", None, (1, 100), "Taubin-smoothed mesh {idx}_mesh_smooth.ply / .txt: the iterations (ops.mesh_smooth)", "absent"),
    ("smooth_lambda", 0.5, (0.0, 1.0), "... the positive step lambda", "str"),
    ("smooth_band", 0.1, (0.0, 0.5), "... Taubin's pass-band k_PB: the negative step is mu = 1 / (smooth_band - 1 / smooth_lambda)", "str"),
))
# The refinement of the written mesh, in a table of its own with the same rows: MESH_TABLE stays the smoothing's three.
MESH_SUBDIVIDE_TABLE = tuple(Setting(*row) for row in (
    ("subdivide", None, (1, 3), "Loop-subdivided mesh {idx}_mesh_subdiv.ply / .txt projected onto the SDF: the levels (ops.mesh_subdivide)", "absent"),
    ("subdivide_project", 2, (0, 8), "... the Newton steps onto the network's zero set after the subdivision (ops.mesh_project_step); 0 = none"),
))
MESH = {row.key: row for row in MESH_TABLE + MESH_SUBDIVIDE_TABLE}


def mesh_setting(opt, key):
    """opt.mesh[key] checked against its row of MESH_TABLE or MESH_SUBDIVIDE_TABLE, the row's default where the option tree has no such
    key or no `mesh` group."""
    row = MESH[key]
    return _checked("mesh", row, (opt.get("mesh", None) or {}).get(key, row.default))


def smooth_settings(opt):
    """None unless `--mesh.smooth=n` is given, else (n, lam, mu), the arguments of ops.mesh_smooth.  A pair with mu <= -1 is refused,
    switch on or off: the negative step would amplify the highest frequency of the umbrella operator."""
    iters, lam, band = (mesh_setting(opt, k) for k in ("smooth", "smooth_lambda", "smooth_band"))
    mu = 1.0 / (band - 1.0 / lam)
    if mu <= -1.0:
        raise ValueError("mesh.smooth_lambda = %r and mesh.smooth_band = %r give mu = %.6g <= -1: choose mesh.smooth_lambda < "
                         "1 / (1 + mesh.smooth_band) = %.6g" % (lam, band, mu, 1.0 / (1.0 + band)))
    return None if iters is None else (iters, lam, mu)


def subdivide_settings(opt):
    """None unless `--mesh.subdivide=n` is given, else (levels, project): the levels of ops.mesh_subdivide and the Newton steps of
    eval_3D.meshes_subdivided.  Both values are checked, switch on or off."""
    levels, project = (mesh_setting(opt, k) for k in ("subdivide", "subdivide_project"))
    return None if levels is None else (levels, project)


# The checks of the written meshes, in a table and a dict of their own (MESH stays the post-processing steps' five rows): a check
# changes no mesh and writes no mesh of its own, only a sidecar that says what it found.
MESH_CHECK_TABLE = tuple(Setting(*row) for row in (
    ("self_intersect", False, bool, "pairs of faces that properly cross, per written mesh: {idx}_mesh_selfx.txt and the hit faces "
                                    "{idx}_mesh_selfx_{variant}.ply (ops.mesh_self_intersections)"),
))
MESH_CHECK = {row.key: row for row in MESH_CHECK_TABLE}


def self_intersect_settings(opt):
    """`--mesh.self_intersect`, a bool; absent (the key or the whole `mesh` group) means off."""
    row = MESH_CHECK["self_intersect"]
    return _checked("mesh", row, (opt.get("mesh", None) or {}).get(row.key, row.default))


# The decimation of the written mesh to a face budget, in a table and a dict of their own with the same rows (MESH stays the five rows
# of smoothing and refinement).
MESH_DECIMATE_TABLE = tuple(Setting(*row) for row in (
    ("decimate", None, (4, 16777216), "edge-collapse mesh {idx}_mesh_decimated.ply / .txt: the face budget (ops.mesh_decimate)", "absent"),
    ("decimate_reg", 1e-3, (0.0, 1.0), "... the pull of a collapse's vertex towards the midpoint of its edge", "str"),
    ("decimate_rounds", 1024, (1, 4096), "... the most rounds of independent collapses"),
))
MESH_DECIMATE = {row.key: row for row in MESH_DECIMATE_TABLE}


def decimate_settings(opt):
    """None unless `--mesh.decimate=F` is given, else (target, reg, rounds), the arguments of ops.mesh_decimate.  All three values are
    checked, switch on or off; absent (a key or the whole `mesh` group) means the default."""
    target, reg, rounds = (_checked("mesh", MESH_DECIMATE[k], (opt.get("mesh", None) or {}).get(k, MESH_DECIMATE[k].default))
                           for k in ("decimate", "decimate_reg", "decimate_rounds"))
    return None if target is None else (target, reg, rounds)


# The shading of what is written for a viewer, in a table and a dict of their own with the same rows (the tables above stay as they are):
# ambient occlusion baked from the level grid changes no mesh and measures nothing; it adds files beside the ones that are written.
MESH_SHADE_TABLE = tuple(Setting(*row) for row in (
    ("ao", False, bool, "ambient occlusion from the level grid: {idx}_mesh_ao.ply / .txt, an AO atlas beside --eval.texture and shaded pictures "
                        "beside --eval.mesh_render (ops.level_ambient_occlusion)"),
    ("ao_radius", 0.125, (0.0, 1.0), "... the reach of a ray as a fraction of the grid's S - 1 pitches", "str"),
))
MESH_SHADE = {row.key: row for row in MESH_SHADE_TABLE}


def ao_settings(opt, S=None):
    """None unless `--mesh.ao` is set, else the reach of ops.level_ambient_occlusion: mesh.ao_radius (S - 1) grid pitches for a level grid
    of S points per axis, the fraction mesh.ao_radius itself while S is None.  Both values are checked, switch on or off; absent (a key
    or the whole `mesh` group) means the default."""
    on, radius = (_checked("mesh", MESH_SHADE[k], (opt.get("mesh", None) or {}).get(k, MESH_SHADE[k].default)) for k in ("ao", "ao_radius"))
    if not on:
        return None
    return radius if S is None else radius * (int(S) - 1)


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
    for check in (dual_mesh_reg, texture_texels, mesh_render, icp_settings, normal_settings, mesh_dist_settings, emd_settings, iou_settings,
                  mesh_stats_settings, simplify_settings,       # every eval.* value is checked here, whether or not its switch is on
                  smooth_settings, subdivide_settings, self_intersect_settings, decimate_settings, ao_settings):    # and every mesh.* value
        check(opt)
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
