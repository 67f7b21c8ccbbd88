"""CLIP-annotation mode of data/pix3d.py and its preprocessing (data/clip_preprocess.py), no GPU:
  * the loader's samples and path lists equal what the reference's own loader produced on the miniature tree (golden G18,
    tests/golden/make_golden_pix3d_clip.py), bit for bit, in both preprocessing modes' CPU halves;
  * the coefficient builder + a numpy resample equal PIL.Image.resize(BICUBIC);
  * a numpy restatement of the kernel's integer arithmetic on kernel_tables equals the CPU chain (tables, crop, quantisation);
  * resize-size and crop-offset arithmetic; only a ClipPreprocess transform is accepted."""
import os

import numpy as np
import PIL.Image
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _opt(root, extra=()):
    from shapeclipper_amd.utils import options
    return options.set(options.parse_arguments(["--yaml=%s/options/clip/pix3d.yaml" % ROOT, "--name=pix3d_clip",
                                                "--output_root=/tmp/sc_pix3d_clip", "--data.pix3d.cat=chair,sofa",
                                                "--data.pix3d.root=%s" % root, "--data.num_workers=0"] + list(extra)), verbose=False)


@pytest.fixture(scope="module")
def golden_tree(tmp_path_factory):
    from shapeclipper_amd.data import pix3d_mini
    root = str(tmp_path_factory.mktemp("g18") / "Pix3D")
    pix3d_mini.write_tree(root, n_per_cat=3, k_nearest=2, cat_key="chair,sofa", n_points=64)     # make_golden_pix3d_clip.py's tree
    return root


def _kernel_numpy(rgba, n_px, bgcolor):
    """csrc/clip_preprocess.hip's arithmetic in numpy: quantise, horizontal and vertical passes over kernel_tables, normalise."""
    from shapeclipper_amd.data import clip_preprocess as cp
    H, W, _ = rgba.shape
    hb, hk, vb, vk = cp.kernel_tables(H, W, n_px)
    bg = cp.background_byte(bgcolor)
    q = rgba[..., :3].astype(np.int64)
    if bg >= 0:
        q = np.where(rgba[..., 3:] >= 128, q, bg)
    tmp = cp.resample_axis(q.astype(np.uint8), hb, hk, axis=1)            # [H, n_px, 3]
    v = cp.resample_axis(tmp, vb, vk, axis=0)                             # [n_px, n_px, 3]
    x = torch.from_numpy(v).permute(2, 0, 1).float().div(255)
    return x.sub(torch.tensor(cp.MEAN)[:, None, None]).div(torch.tensor(cp.STD)[:, None, None])


@pytest.mark.parametrize("device_pre", [False, True])
@pytest.mark.parametrize("case", ["s224", "s64x86"])
def test_clip_mode_equals_the_reference_loader(golden, golden_tree, case, device_pre):
    import data.pix3d as pix3d
    from shapeclipper_amd.data.clip_preprocess import ClipPreprocess
    g = golden("g18_pix3d_clip")
    H, W, bg = g["%s/config" % case]
    bg = float(bg)
    opt = _opt(golden_tree, ["--image_size=[%d,%d]" % (H, W), "--data.bgcolor=%s" % bg]
               + ([] if device_pre else ["--hip.device_clip_preprocess!"]))
    pre = ClipPreprocess(224, opt.data.bgcolor)
    ds = pix3d.Dataset(opt, split="train", transform=pre)
    assert ds.clip_anno and not hasattr(ds, "NN_dict")
    assert ds.rel_path_list == g["%s/rel_path_list" % case].tolist()
    assert [p.replace(golden_tree, "data/Pix3D") for p in ds.img_path_list] == g["%s/img_path_list" % case].tolist()
    assert [p.replace(golden_tree, "data/Pix3D") for p in ds.pc_path_list] == g["%s/pc_path_list" % case].tolist()
    table = torch.from_numpy(g["norm_table"])
    idxs = sorted({int(k.split("/")[1]) for k in g.files if k.startswith(case + "/") and k.split("/")[1].isdigit()})
    assert idxs == [0, 2]
    for i in idxs:
        u8 = torch.from_numpy(g["%s/%d/u8" % (case, i)].astype(np.int64)).permute(2, 0, 1)
        want = table[torch.arange(3)[:, None, None], u8]
        s = ds[i]
        if device_pre:
            assert sorted(s) == ["idx", "rgba_input"] and s["idx"] == i
            rgba = s["rgba_input"]
            assert rgba.dtype == torch.uint8 and rgba.shape == (H, W, 4)
            got = _kernel_numpy(rgba.numpy(), 224, bg)                     # what the kernel computes from this sample
            assert torch.equal(pre(PIL.Image.fromarray(rgba.numpy(), "RGBA")), want)
        else:
            assert sorted(s) == ["idx", "rgb_input"] and s["idx"] == i
            got = s["rgb_input"]
        assert got.dtype == torch.float32 and got.shape == (3, 224, 224)
        assert torch.equal(got, want), (case, i)


@pytest.mark.parametrize("src,dst", [((64, 64), (224, 224)), ((300, 300), (224, 224)), ((96, 128), (298, 224)),
                                     ((400, 500), (179, 224)), ((80, 96), (80, 200)), ((80, 96), (300, 96)), ((5, 7), (224, 313))])
def test_coefficients_match_pillow_bicubic(src, dst):
    from shapeclipper_amd.data import clip_preprocess as cp
    rng = np.random.RandomState(sum(src) + sum(dst))
    img = rng.randint(0, 256, src + (3,)).astype(np.uint8)
    want = np.array(PIL.Image.fromarray(img).resize(dst[::-1], PIL.Image.BICUBIC))
    assert np.array_equal(cp.resize_numpy(img, dst[::-1]), want)


def test_coefficient_tables_follow_pillows_recipe():
    from shapeclipper_amd.data import clip_preprocess as cp
    bounds, kk = cp.bicubic_coeffs(64, 224)                  # upscale: support 2, ksize 5
    assert kk.shape == (224, 5) and kk.dtype == np.int32
    assert (bounds[:, 0] >= 0).all() and (bounds.sum(1) <= 64).all() and bounds[0].tolist() == [0, 2]
    assert (np.abs(kk.sum(1) - (1 << 22)) <= 5).all()
    bounds, kk = cp.bicubic_coeffs(500, 224)                 # downscale: support 2 * 500 / 224
    assert kk.shape == (224, 2 * int(np.ceil(2 * 500 / 224)) + 1)


def test_resize_size_and_crop_offsets():
    from shapeclipper_amd.data.clip_preprocess import crop_offsets, resize_size
    assert resize_size(224, 224, 224) == (224, 224)
    assert resize_size(64, 64, 224) == (224, 224)
    assert resize_size(64, 86, 224) == (224, 301)            # int(224 * 86 / 64) = int(301.0)
    assert resize_size(86, 64, 224) == (301, 224)
    assert resize_size(60, 80, 224) == (224, 298)            # int(298.67)
    assert resize_size(500, 400, 224) == (280, 224)
    assert crop_offsets(224, 301, 224) == (0, 38)            # 38.5: Python's round, half to even
    assert crop_offsets(224, 299, 224) == (0, 38)            # 37.5 -> 38
    assert crop_offsets(298, 224, 224) == (37, 0)
    assert crop_offsets(224, 224, 224) == (0, 0)


@pytest.mark.parametrize("hw", [(224, 224), (64, 86), (96, 80), (300, 260), (224, 298)])
@pytest.mark.parametrize("bgcolor", [1, 0, 0.5, None])
def test_kernel_arithmetic_equals_the_cpu_chain(hw, bgcolor):
    from shapeclipper_amd.data.clip_preprocess import ClipPreprocess
    H, W = hw
    rng = np.random.RandomState(H * 7 + W)
    rgba = rng.randint(0, 256, (H, W, 4)).astype(np.uint8)
    rgba[0, :, 3] = 127
    rgba[1, :, 3] = 128
    want = ClipPreprocess(224, bgcolor)(PIL.Image.fromarray(rgba, "RGBA"))
    assert torch.equal(_kernel_numpy(rgba, 224, bgcolor), want)


def test_background_byte_truncates():
    from shapeclipper_amd.data.clip_preprocess import background_byte
    assert [background_byte(b) for b in (1, 0, 0.5, None, 0.999)] == [255, 0, 127, -1, 254]
    with pytest.raises(ValueError):
        __import__("shapeclipper_amd.data.clip_preprocess", fromlist=["x"]).ClipPreprocess(224, 2)


def test_only_clip_preprocess_is_accepted(golden_tree):
    import data.pix3d as pix3d
    from shapeclipper_amd.data.clip_preprocess import ClipPreprocess
    opt = _opt(golden_tree)
    assert pix3d.Dataset(opt, split="train", transform=ClipPreprocess(224, 1)).clip_anno
    for bad in (lambda x: x, "clip"):
        with pytest.raises(NotImplementedError, match="CLIP-annotation"):
            pix3d.Dataset(opt, split="train", transform=bad)


def test_clip_mode_collates_with_workers(golden_tree):
    import data.pix3d as pix3d
    from shapeclipper_amd.data.clip_preprocess import ClipPreprocess
    opt = _opt(golden_tree, ["--image_size=[48,64]"])
    ds = pix3d.Dataset(opt, split="train", transform=ClipPreprocess(224, 1))
    loader = torch.utils.data.DataLoader(ds, batch_size=4, num_workers=2, shuffle=False, drop_last=False)
    batches = list(loader)
    assert [b["rgba_input"].shape for b in batches] == [(4, 48, 64, 4), (2, 48, 64, 4)]
    assert torch.cat([b["idx"] for b in batches]).tolist() == list(range(6))


def test_the_c_entry_point_refuses_bad_arguments_without_launching():
    import ctypes
    from shapeclipper_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    ok = dict(n=1, H=64, W=86, n_px=224, bg=255, h_taps=5, v_taps=5)
    bad = [dict(n=-1), dict(H=0), dict(W=16385), dict(n_px=0), dict(n_px=2049), dict(bg=256), dict(bg=-2), dict(h_taps=0),
           dict(v_taps=1025), dict(n=65536), dict()]                # the last one: NULL pointers
    for b in bad:
        a = dict(ok, **b)
        code = lib.sc_clip_preprocess(null, a["n"], a["H"], a["W"], a["n_px"], a["bg"], null, null, a["h_taps"], null, null, a["v_taps"],
                                      null, null, null)
        assert code == 1, b                                         # hipErrorInvalidValue
    assert lib.sc_clip_preprocess(null, 0, 64, 86, 224, 255, null, null, 5, null, null, 5, null, null, null) == 0
