"""Training-time visualisation (`--hip.train_vis`), the host side: the visualisation samples (reference runner.py:60-111), the GIF writer and
the pose axes of utils/util_vis.py, the mask colouring the frame kernel states, and the switch's default.  No GPU."""
import io
import os
import types

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_the_switch_is_off_by_default():
    from shapeclipper_amd.utils import options
    assert options.HIP_DEFAULTS["hip"]["train_vis"] is False


# ---- append_viz_data -------------------------------------------------------------------------------------------------------
def _fake_batches(labels, batch_size):
    out = []
    for s in range(0, len(labels), batch_size):
        lab = torch.tensor(labels[s:s + batch_size])
        n = len(lab)
        out.append(dict(idx=torch.arange(s, s + n), category_label=lab, rgb_input_map=torch.arange(s, s + n).float().view(n, 1, 1, 1).expand(n, 3, 2, 2),
                        dpc=dict(points=torch.arange(s, s + n).float().view(n, 1, 1).expand(n, 4, 3))))
    return out


def _runner_with(batches):
    from shapeclipper_amd.model.runner import Runner
    runner = Runner.__new__(Runner)                 # no output directory, no data set: only the visualisation loader is used
    runner.viz_data = []
    runner.viz_loader_iter = iter(batches)
    return runner


@pytest.mark.parametrize("batch_size", [1, 3])
def test_append_viz_data_takes_one_sample_per_category_until_n_vis_classes(batch_size):
    from shapeclipper_amd.utils.util import EasyDict as edict
    labels = [2, 2, 0, 1, 0, 2, 1, 3, 3, 0, 1, 2, 3, 1, 0, 2, 2, 0]
    opt = edict(data=edict(num_classes=4), eval=edict(n_vis_classes=3))
    runner = _runner_with(_fake_batches(labels, batch_size))
    for _ in range(2):                               # n_vis = 2
        runner.append_viz_data(opt)
    # a restatement of the reference's loop over the same stream
    want, pos = [], 0
    for _ in range(2):
        seen = [0] * 4
        while sum(seen) < 3:
            batch = labels[pos:pos + batch_size]
            for k, c in enumerate(batch):
                if not seen[c]:
                    seen[c] += 1
                    want.append(pos + k)
            pos += len(batch)
    assert [int(s["idx"]) for s in runner.viz_data] == want
    for s in runner.viz_data:
        i = int(s["idx"])
        assert s["idx"].shape == (1,) and s["category_label"].shape == (1,) and int(s["category_label"]) == labels[i]
        assert s["rgb_input_map"].shape == (1, 3, 2, 2) and float(s["rgb_input_map"][0, 0, 0, 0]) == i
        assert s["dpc"]["points"].shape == (1, 4, 3) and float(s["dpc"]["points"][0, 0, 0]) == i


def test_append_viz_data_caps_n_vis_classes_at_the_number_of_classes():
    from shapeclipper_amd.utils.util import EasyDict as edict
    opt = edict(data=edict(num_classes=2), eval=edict(n_vis_classes=10))
    runner = _runner_with(_fake_batches([1, 1, 0, 1, 0], 1))
    runner.append_viz_data(opt)
    assert [int(s["idx"]) for s in runner.viz_data] == [0, 2]
    opt = edict(data=edict(num_classes=2), eval=edict())              # no n_vis_classes: all classes
    runner = _runner_with(_fake_batches([0, 0, 1], 1))
    runner.append_viz_data(opt)
    assert [int(s["idx"]) for s in runner.viz_data] == [0, 2]


# ---- load_dataset: the visualisation loader exists only with the switch -------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from shapeclipper_amd.data import pix3d_mini
    root = str(tmp_path_factory.mktemp("vis") / "Pix3D")
    pix3d_mini.write_tree(root, n_per_cat=3, k_nearest=2, cat_key="chair,sofa", n_points=64)
    return root


def _opt(tree, tmp, extra=()):
    from shapeclipper_amd.utils import options
    opt = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=train_vis", "--output_root=%s" % tmp,
                                               "--data.pix3d.cat=chair,sofa", "--data.num_classes=2", "--data.pix3d.root=%s" % tree,
                                               "--data.k_nearest=2", "--data.num_workers=0", "--image_size=[32,32]", "--batch_size=2",
                                               "--eval.n_vis=1"] + list(extra)), verbose=False)
    opt.device, opt.world_size = "cpu", 1
    return opt


def test_load_dataset_without_the_switch_leaves_the_cpu_generator_alone(tree, tmp_path):
    from shapeclipper_amd.model.runner import Runner
    opt = _opt(tree, tmp_path)
    torch.manual_seed(123)
    state = torch.get_rng_state()
    runner = Runner(opt)
    runner.load_dataset(opt, eval_split="test")
    assert torch.equal(torch.get_rng_state(), state)
    assert runner.viz_data == [] and not hasattr(runner, "viz_loader")


def test_load_dataset_with_the_switch_picks_the_samples_as_the_reference_does(tree, tmp_path):
    from shapeclipper_amd.model.runner import Runner
    opt = _opt(tree, tmp_path, ["--hip.train_vis"])
    torch.manual_seed(123)
    state = torch.get_rng_state()
    runner = Runner(opt)
    runner.load_dataset(opt, eval_split="test")
    assert not torch.equal(torch.get_rng_state(), state)            # the shuffled loader's sampler drew its seed
    assert sorted(int(s["category_label"]) for s in runner.viz_data) == [0, 1]
    # the same picks as a shuffled loader over the test split created and iterated at that point of the generator's stream
    torch.set_rng_state(state)
    import data.pix3d as pix3d
    ds = pix3d.Dataset(opt, split="test")
    order = [int(b["idx"]) for b in ds.setup_loader(opt, shuffle=True, drop_last=False, batch_size=1)]
    labels = [int(ds.cat2label[ds.list[i][0]]) for i in order]
    first = [order[labels.index(c)] for c in sorted(set(labels), key=labels.index)]
    assert [int(s["idx"]) for s in runner.viz_data] == first
    assert runner.viz_data[0]["rgb_input_map"].shape == (1, 3, 32, 32)


# ---- util_vis ----------------------------------------------------------------------------------------------------------------------
def _opt_out(tmp_path):
    os.makedirs(tmp_path / "vis", exist_ok=True)
    return types.SimpleNamespace(output_path=str(tmp_path))


def test_dump_gifs_writes_what_pil_writes(tmp_path):
    from PIL import Image
    from shapeclipper_amd.utils import util_vis
    rng = np.random.RandomState(0)
    frames = rng.randint(0, 256, (2, 50, 16, 12, 3)).astype(np.uint8)
    util_vis.dump_gifs(_opt_out(tmp_path), torch.tensor([7, 3]), "image_rotate", torch.from_numpy(frames), folder="vis")
    for i, clip in zip((7, 3), frames):
        fname = tmp_path / "vis" / ("%d_image_rotate.gif" % i)
        images = [Image.fromarray(f).convert("RGB") for f in clip]
        want = io.BytesIO()
        images[0].save(want, format="GIF", append_images=images[1:], save_all=True, duration=100, loop=0)
        assert fname.read_bytes() == want.getvalue()
        gif = Image.open(fname)
        assert gif.n_frames == 50 and gif.info["loop"] == 0
        durations = []
        for k in range(gif.n_frames):
            gif.seek(k)
            durations.append(gif.info["duration"])
        assert durations == [100] * 50


def _reference_pose_chain(image, rot, size=20, width=2):
    """Reference utils/util_vis.py:54-65 + draw_pose :112-129 for an RGB float image [3,H,W] in [0, 1], restated without torchvision:
    to_pil_image = mul(255).byte() -> PIL; draw; alpha_composite; to_tensor = byte / 255; then (img * 255).astype(np.uint8)."""
    from PIL import Image, ImageDraw
    pil = Image.fromarray(image.mul(255).byte().permute(1, 2, 0).numpy(), mode="RGB").convert("RGBA")
    layer = Image.new("RGBA", pil.size, (0, 0, 0, 0))
    draw = ImageDraw.Draw(layer)
    center = (size, size)
    endpoint = [(size + size * p[0], size + size * p[1]) for p in rot.t()]
    draw.line([center, endpoint[0]], fill=(255, 0, 0), width=width)
    draw.line([center, endpoint[1]], fill=(0, 255, 0), width=width)
    draw.line([center, endpoint[2]], fill=(0, 0, 255), width=width)
    pil.alpha_composite(layer)
    back = torch.from_numpy(np.array(pil.convert("RGB"))).permute(2, 0, 1).float().div(255)
    return (back.permute(1, 2, 0).contiguous().numpy() * 255).astype(np.uint8)


def test_dump_images_draws_the_pose_axes_as_the_reference(tmp_path):
    from PIL import Image
    from shapeclipper_amd.model.graph import rotation_from_trig
    from shapeclipper_amd.utils import util_vis
    g = torch.Generator().manual_seed(2)
    B = 3
    images = torch.rand(B, 3, 40, 48, generator=g) * 1.2 - 0.1
    trig = lambda t: torch.stack([torch.cos(t), torch.sin(t)], 1)
    rot = rotation_from_trig(trig(torch.rand(B, generator=g) * 6), trig(torch.rand(B, generator=g) - 0.5), trig(torch.rand(B, generator=g)))
    poses = torch.cat([rot, torch.rand(B, 3, 1, generator=g)], 2)
    opt = _opt_out(tmp_path)
    util_vis.dump_images(opt, torch.tensor([4, 5, 6]), "image_recon", images, poses=poses, folder="vis")
    util_vis.dump_images(opt, torch.tensor([4, 5, 6]), "image_plain", images, folder="vis")
    for k, i in enumerate((4, 5, 6)):
        got = np.array(Image.open(tmp_path / "vis" / ("%d_image_recon.png" % i)))
        want = _reference_pose_chain(images[k].clamp(0, 1), poses[k, :, :3])
        assert got.shape == want.shape and np.array_equal(got, want), i
        plain = np.array(Image.open(tmp_path / "vis" / ("%d_image_plain.png" % i)))
        assert not np.array_equal(plain, got)                         # the axes were drawn
        assert np.array_equal(plain[30:, 30:], got[30:, 30:])        # ... in the corner only


# ---- the mask colouring of csrc/vis_frames.hip ------------------------------------------------------------------------------------
def mask_bytes(x):
    """sc_vis_frames' mask formula (kind 1), restated: clamp to [0, 1], trunc(v * 256) with 256 -> 255, NaN -> 0."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        v = np.clip(x, np.float32(0), np.float32(1))
        i = np.minimum(np.trunc(v * np.float32(256)), 255)
    i[np.isnan(x)] = 0
    return np.repeat(i.astype(np.uint8)[:, None], 3, axis=1)


def test_mask_formula_equals_matplotlib_gray_as_get_heatmap_applies_it(golden):
    g = golden("vis_gray_lut")
    # the table's 8-bit round trip (float64 -> fp32 -> * 255 -> trunc) is the identity on the index ...
    lut = g["lut_rgb"].astype(np.float32)
    assert np.array_equal((lut * np.float32(255)).astype(np.uint8), np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1))
    assert np.array_equal(g["bad_rgb"], [0, 0, 0])
    # ... so the kernel's bytes are the index, on every probe: the k / 256 edges and their neighbours, out-of-range values, +-inf, NaN
    assert np.array_equal(mask_bytes(g["x"]), g["bytes"])
    # and it is not the RGB formula
    half = np.float32(0.5)
    assert mask_bytes([half])[0, 0] == 128 and int(half * np.float32(255)) == 127


def test_vis_frames_refuses_host_tensors_and_bad_shapes():
    from shapeclipper_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.vis_frames(torch.zeros(4, 3), "rgb")
    with pytest.raises(ValueError):
        ops.vis_frames(torch.zeros(4, 3), "mask")
    with pytest.raises(ValueError):
        ops.vis_frames(torch.zeros(4, 1), "depth")
