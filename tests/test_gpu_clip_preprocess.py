"""CLIP preprocessing on the device (csrc/clip_preprocess.hip via ops.clip_preprocess) and the Pix3D path of CLIP_anno.py:
  * ops.clip_preprocess equals the CPU chain (data/clip_preprocess.ClipPreprocess, the reference's composite + CLIP preprocess)
    bit for bit: identity, upscale, downscale, non-square and half-pixel-crop sizes; bgcolor 1, 0, 0.5, None; alpha 127 / 128;
  * CLIP_anno.main() on a miniature Pix3D tree with ViT-B/32 and batches smaller than a split: three CSVs in the reference's format,
    byte-identical with and without --hip.device_clip_preprocess, the three CLIP_NN_{split}.png, and the training loader reads the CSVs."""
import csv
import os
import sys

import numpy as np
import PIL.Image
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _images(B, H, W, seed):
    rng = np.random.RandomState(seed)
    rgba = rng.randint(0, 256, (B, H, W, 4)).astype(np.uint8)
    rgba[:, 0::3, :, 3] = 127                                    # the threshold: a / 255 > 0.5 <=> a >= 128
    rgba[:, 1::3, :, 3] = 128
    rgba[:, :, 0, 3] = 0
    rgba[:, :, -1, 3] = 255
    return rgba


@pytest.mark.parametrize("hw", [(224, 224), (64, 86), (86, 64), (96, 80), (300, 260), (224, 298), (500, 400), (1, 1)])
@pytest.mark.parametrize("bgcolor", [1, 0, 0.5, None])
def test_device_preprocess_equals_the_cpu_chain(hw, bgcolor):
    from shapeclipper_amd import ops
    from shapeclipper_amd.data.clip_preprocess import ClipPreprocess
    H, W = hw
    B = 3
    rgba = _images(B, H, W, H * 31 + W)
    pre = ClipPreprocess(224, bgcolor)
    got = pre.device(torch.from_numpy(rgba).cuda())
    torch.cuda.synchronize()
    assert got.shape == (B, 3, 224, 224) and got.dtype == torch.float32
    want = torch.stack([pre(PIL.Image.fromarray(rgba[b], "RGBA")) for b in range(B)])
    assert torch.equal(got.cpu(), want)
    # the wrapper builds the same tables itself
    assert torch.equal(ops.clip_preprocess(torch.from_numpy(rgba).cuda(), 224, bgcolor).cpu(), want)


def test_other_output_sizes_and_empty_batches():
    from shapeclipper_amd import ops
    from shapeclipper_amd.data.clip_preprocess import ClipPreprocess
    rgba = _images(2, 50, 70, 7)
    for n_px in (32, 49, 336):
        pre = ClipPreprocess(n_px, 1)
        want = torch.stack([pre(PIL.Image.fromarray(r, "RGBA")) for r in rgba])
        assert torch.equal(pre.device(torch.from_numpy(rgba).cuda()).cpu(), want), n_px
    out = ops.clip_preprocess(torch.zeros(0, 50, 70, 4, dtype=torch.uint8, device="cuda"), 224, 1)
    assert out.shape == (0, 3, 224, 224)
    with pytest.raises(ValueError):
        ops.clip_preprocess(torch.zeros(1, 50, 70, 3, dtype=torch.uint8, device="cuda"), 224, 1)
    with pytest.raises(ValueError):
        ops.clip_preprocess(torch.zeros(1, 50, 70, 4, dtype=torch.uint8, device="cuda"), 4096, 1)


def _tree(tmp_path):
    """The miniature tree with val / train / test lists, without the sample names that contain "img" / "mask": the reference's
    str.replace renames those in rel_path_list (golden G18 pins that), so the training loader could not find them again."""
    from shapeclipper_amd.data import pix3d_mini
    root = str(tmp_path / "Pix3D")
    pix3d_mini.write_tree(root, n_per_cat=6, k_nearest=5, cat_key="chair,sofa", n_points=64, splits=("train", "val", "test"))
    for f in os.listdir(os.path.join(root, "lists")):
        p = os.path.join(root, "lists", f)
        names = [n for n in open(p).read().splitlines() if "img" not in n]
        with open(p, "w") as fh:
            fh.write("\n".join(names) + "\n")
    return root


def _run(monkeypatch, root, anno_root, out_root, extra=()):
    import CLIP_anno
    argv = ["CLIP_anno.py", "--yaml=%s/options/clip/pix3d.yaml" % ROOT, "--data.pix3d.root=%s" % root, "--data.pix3d.cat=chair,sofa",
            "--anno_root=%s" % anno_root, "--output_root=%s" % out_root, "--clip_model=ViT-B/32", "--batch_size=4",
            "--data.num_workers=2", "--image_size=[96,128]"] + list(extra)
    monkeypatch.setattr(sys, "argv", argv)
    torch.manual_seed(0)
    CLIP_anno.main()
    return CLIP_anno.options.set(opt_cmd=CLIP_anno.options.parse_arguments(argv[1:]), verbose=False)


def test_clip_anno_on_pix3d(tmp_path, monkeypatch):
    import data.pix3d as pix3d
    from shapeclipper_amd.data.clip_preprocess import ClipPreprocess
    root = _tree(tmp_path)
    k = 6
    dev_anno, cpu_anno = str(tmp_path / "anno_dev"), str(tmp_path / "anno_cpu")
    opt = _run(monkeypatch, root, dev_anno, str(tmp_path / "out_dev"))
    _run(monkeypatch, root, cpu_anno, str(tmp_path / "out_cpu"), ["--hip.device_clip_preprocess!"])
    splits = ("val", "train", "test")
    assert sorted(os.listdir(dev_anno)) == sorted("chair,sofa_%s.csv" % s for s in splits)
    assert sorted(f for f in os.listdir(opt.output_path) if f.endswith(".png")) == sorted("CLIP_NN_%s.png" % s for s in splits)
    for s in splits:
        png = PIL.Image.open(os.path.join(opt.output_path, "CLIP_NN_%s.png" % s))
        assert png.size == (100 * 5 * k, 100 * 5 * 15)
        a = open(os.path.join(dev_anno, "chair,sofa_%s.csv" % s), "rb").read()
        assert a == open(os.path.join(cpu_anno, "chair,sofa_%s.csv" % s), "rb").read(), s
        rows = list(csv.reader(open(os.path.join(dev_anno, "chair,sofa_%s.csv" % s))))
        header, body = rows[0], rows[1:]
        assert header == ["Query"] + ["Top_%d" % i for i in range(1, k)] + ["Top_%d_score" % i for i in range(1, k)]
        labels = pix3d.Dataset(opt, split=s, transform=ClipPreprocess(224, 1)).rel_path_list
        assert len(labels) == 10 and [r[0] for r in body] == sorted(labels)
        for r in body:
            assert len(r) == 1 + 2 * (k - 1) and r[0] not in r[1:k] and set(r[1:k]) <= set(labels)
            scores = [float(v) for v in r[k:]]
            assert scores == sorted(scores, reverse=True) and all(len(v.split(".")[1]) == 4 for v in r[k:])
    # the training loader reads the new CSVs from <root>/CLIP_NN
    import shutil
    for s in splits:
        shutil.copy(os.path.join(dev_anno, "chair,sofa_%s.csv" % s), os.path.join(root, "CLIP_NN", "chair,sofa_%s.csv" % s))
    from shapeclipper_amd.utils import options
    topt = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=clip_anno_train",
                                                "--output_root=%s/train" % tmp_path, "--data.pix3d.cat=chair,sofa",
                                                "--data.pix3d.root=%s" % root, "--image_size=[32,32]", "--data.k_nearest=5"]),
                       verbose=False)
    ds = pix3d.Dataset(topt, split="train")
    rows = {r[0]: r for r in csv.reader(open(os.path.join(dev_anno, "chair,sofa_train.csv")))}
    for i in range(len(ds)):
        c, name = ds.list[i]
        assert ds.NN_dict[(c, name)] == [tuple(p.split(".")[0].split("/")) for p in rows["%s/%s.png" % (c, name)][1:k]]
    s = ds[0]
    assert s["rgb_input_map_NN"].shape == (3, 32, 32, 5)
