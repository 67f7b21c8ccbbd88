"""Training-time visualisation on the device (`--hip.train_vis`):
  * ops.vis_frames (csrc/vis_frames.hip) equals a restatement of the reference's float -> uint8 recipe bit for bit, for the three kinds
    of frame, on random, out-of-range, exactly 0 / 1 and NaN values;
  * the batched turn-table (Runner.vis_rotate(batched=True) -> Renderer.render_views) equals the reference's per-view loop bit for bit,
    for any chunking of the views, and leaves the CPU generator where the loop leaves it;
  * train.py (its entry point, in this process) with --hip.train_vis on a miniature Pix3D tree writes vis_0/ and vis_log/iter_{it}/ as the reference names them, and
    writes no vis* folder without the switch."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- ops.vis_frames ---------------------------------------------------------------------------------------------------------------
def _values(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g) * 1.6 - 0.3                    # in range and out of range on both sides
    flat = x.view(-1)
    n = flat.numel()
    special = torch.tensor([0.0, 1.0, -0.0, 0.5, float("nan"), float("inf"), -float("inf"), -1.0, 2.0, 1.0 - 2 ** -24, 2 ** -24])
    for k, v in enumerate(special):
        flat[torch.arange(k, n, 97)] = v
    edges = flat[11::13]                                                # the k / 256 mask edges
    edges.copy_(torch.arange(edges.numel()).float().remainder(257) / 256)
    return x


def _reference_rgb(x_dev, lo, hi):
    """preprocess_vis_image on the device (reference utils/util_vis.py:35-44), then (img * 255).astype(np.uint8) -- NaN written as 0."""
    v = ((x_dev - lo) / (hi - lo)).clamp(min=0, max=1).cpu().numpy()
    nan = np.isnan(v)
    v[nan] = 0
    return (v * 255).astype(np.uint8)


def _reference_mask(x_dev, lut):
    """preprocess_vis_image + get_heatmap (matplotlib's Colormap.__call__ on floats: * N, N -> N - 1, NaN -> the bad colour) with the
    table of tests/golden/vis_gray_lut.npz, float64 -> .float() -> (img * 255).astype(np.uint8)."""
    v = x_dev.clamp(min=0, max=1).cpu().numpy()
    xa = v * np.float32(256)
    xa[xa == 256] = 255
    bad = np.isnan(xa)
    with np.errstate(invalid="ignore"):
        idx = xa.astype(int)
    colour = lut[np.where(bad, 0, idx)]
    colour[bad] = 0
    return (colour.astype(np.float32) * 255).astype(np.uint8)


@pytest.mark.parametrize("shape", [(2, 3, 64, 64), (1, 7, 5), (13,)])
def test_vis_frames_equals_the_reference_recipe(golden, shape):
    from shapeclipper_amd import ops
    lut = golden("vis_gray_lut")["lut_rgb"]
    dev = torch.device("cuda")
    x3 = _values(shape + (3,), 1).to(dev)
    x1 = _values(shape + (1,), 2).to(dev)
    for lo, hi in ((0, 1), (-1, 1)):
        got = ops.vis_frames(x3, "rgb", from_range=(lo, hi))
        assert got.dtype == torch.uint8 and got.shape == shape + (3,)
        assert np.array_equal(got.cpu().numpy(), _reference_rgb(x3, lo, hi)), (lo, hi)
    got = ops.vis_frames(x1, "mask").cpu().numpy()
    assert np.array_equal(got, _reference_mask(x1[..., 0], lut))
    assert np.array_equal(ops.vis_frames(x3, "normal").cpu().numpy(), _reference_rgb(x3 / 2 + 0.5, 0, 1))
    assert ops.vis_frames(x3[:0], "rgb").shape == (0,) + shape[1:] + (3,)


# ---- batched turn-table ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    from shapeclipper_amd.model.graph import Graph
    from shapeclipper_amd.model.implicit import RGBNetwork, SDFNetwork
    from shapeclipper_amd.model.renderer import Renderer
    from shapeclipper_amd.utils import camera, options
    from shapeclipper_amd.utils.util import EasyDict as edict
    dev = torch.device("cuda")
    opt = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=turntable",
                                               "--output_root=/tmp/sc_pytest"]), verbose=False)
    opt.H, opt.W = opt.eval.image_size
    torch.manual_seed(0)
    sdf_net, rgb_net = SDFNetwork(opt), RGBNetwork(opt)
    with torch.no_grad():             # a shape near the geometric initialisation's sphere, colours that vary over it
        for net, scale in ((sdf_net, 0.003), (rgb_net, 0.03)):
            for p in net.parameters():
                p.add_(scale * torch.randn_like(p))
    renderer = Renderer(opt, sdf_net, rgb_net).to(dev)
    B = 2
    var = edict(idx=torch.tensor([3, 8], device=dev), intr=camera.get_intr(opt, torch.tensor([1.0, 1.15])).to(dev),
                scale_dist=torch.tensor([0.9, 1.1], device=dev), proj_latent_sdf=torch.randn(B, 64, device=dev),
                proj_latent_rgb=torch.randn(B, 64, device=dev), rgb_input_map=torch.zeros(B, 3, 2, 2, device=dev))
    Graph.get_rotate_pose(None, opt, var, n_views=50)               # (uses no module state)
    runner = types.SimpleNamespace(graph=types.SimpleNamespace(module=types.SimpleNamespace(renderer=renderer)))
    return opt, runner, var


def _turntable(scene, batched, chunk_views=None):
    from shapeclipper_amd.model.runner import Runner
    opt, runner, var = scene
    var = type(var)(var)
    torch.manual_seed(11)
    Runner.vis_rotate(runner, opt, var, n_views=50, batched=batched, chunk_views=chunk_views)
    torch.cuda.synchronize()
    return var, torch.get_rng_state()


def test_batched_turntable_is_bit_identical_to_the_per_view_loop(scene):
    from shapeclipper_amd.model.runner import Runner
    opt = scene[0]
    ref, ref_state = _turntable(scene, batched=False)
    masks = torch.stack(ref.rotating_masks)
    assert (masks > 0.5).any() and (masks < 0.5).any()              # the shape is in the picture, not all of it
    assert not torch.equal(ref.rotating_imgs[0], ref.rotating_imgs[12])     # the views differ
    ref_frames = Runner.turntable_frames(opt, ref)
    for chunk in (1, 7, 50, None):
        got, state = _turntable(scene, batched=True, chunk_views=chunk)
        assert torch.equal(state, ref_state), chunk
        for key in ("rotating_imgs", "rotating_masks", "rotating_normals"):
            assert len(got[key]) == len(ref[key]) == 50
            for v, (a, b) in enumerate(zip(got[key], ref[key])):
                assert a.shape == b.shape and torch.equal(a, b), (chunk, key, v, (a - b).abs().max().item())
        frames = Runner.turntable_frames(opt, got)                    # raw normals through the kernel's "normal" kind
        for name, f in frames.items():
            assert f.shape == (2, 50, opt.H, opt.W, 3) and torch.equal(f, ref_frames[name]), (chunk, name)


# ---- train.py end to end ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from shapeclipper_amd.data import pix3d_mini
    root = str(tmp_path_factory.mktemp("pix3d_vis") / "Pix3D")
    pix3d_mini.write_tree(root, n_per_cat=6, k_nearest=5, cat_key="chair,sofa", n_points=2000, seed=5, splits=("train", "val", "test"))
    return root


def _train(tree, out, name, extra):
    """train.py's entry point in this process (a launch of another process would have to sort with the subprocess tests of the suite)."""
    from shapeclipper_amd.cli import train_main
    train_main([os.path.join(ROOT, "train.py"), "--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=%s" % name, "--output_root=%s" % out,
                "--arch.enc_pretrained!", "--tb!", "--batch_size=2", "--data.pix3d.cat=chair,sofa", "--data.num_classes=2",
                "--data.pix3d.root=%s" % tree, "--data.num_workers=0", "--data.max_img_cat=2", "--eval.vox_res=16", "--eval.num_points=1000",
                "--eval.n_vis=1", "--max_epoch=1", "--freq.eval=100", "--freq.ckpt_latest=100000", "--freq.scalar=0", "--freq.save_vis=1"]
               + list(extra))
    return os.path.join(out, "pix3d_output", name)


def _gif_ms(fname):
    from PIL import Image
    gif = Image.open(fname)
    total = 0
    for k in range(gif.n_frames):            # (PIL merges identical consecutive frames into one of the summed duration)
        gif.seek(k)
        total += gif.info["duration"]
    return total, gif.info.get("loop")


@pytest.mark.timeout(900)
def test_train_script_writes_the_reference_visualisation(tree, tmp_path):
    out = _train(tree, str(tmp_path), "vis_on", ["--hip.train_vis"])
    vis = os.path.join(out, "vis_0")
    files = sorted(os.listdir(vis))
    ids = sorted({f.split("_")[0] for f in files})
    assert len(ids) == 2, files                                        # n_vis = 1 sample per category, two categories
    pngs = ["image_input", "image_recon", "mask_recon", "mask_input", "normal_input_viewpoint", "normal_input_canonical", "normal_recon"]
    for i in ids:
        for p in pngs:
            assert os.path.getsize(os.path.join(vis, "%s_%s.png" % (i, p))) > 0, (i, p)
        for p in ("mesh", "pointclouds_comp"):
            assert open(os.path.join(vis, "%s_%s.ply" % (i, p)), "rb").read(3) == b"ply", (i, p)
        for g in ("image_rotate", "mask_rotate", "normal_rotate"):
            assert _gif_ms(os.path.join(vis, "%s_%s.gif" % (i, g))) == (50 * 100, 0), (i, g)
    for it in (0, 1):                                                  # two training iterations, freq.save_vis = 1
        logged = sorted(os.listdir(os.path.join(out, "vis_log", "iter_%d" % it)))
        assert logged == sorted("%s_%s.png" % (i, p) for i in ids for p in pngs), logged
    plain = _train(tree, str(tmp_path), "vis_off", [])
    assert not [f for f in os.listdir(plain) if f.startswith("vis")], os.listdir(plain)
