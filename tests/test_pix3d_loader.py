"""data/pix3d.py (the Pix3D loader, reference data/pix3d.py) on the miniature tree of shapeclipper_amd/data/pix3d_mini.py: every key of
its samples is bit-identical to what the reference's own loader produced on the same tree (tests/golden/make_golden_pix3d.py ->
g17_pix3d_loader.npz), and the DataLoader collates with worker processes in both ray modes.  No GPU."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _opt(root, extra=()):
    from shapeclipper_amd.utils import options
    return options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pix3d_loader",
                                                "--output_root=/tmp/sc_pix3d_loader", "--data.pix3d.cat=chair,sofa",
                                                "--data.pix3d.root=%s" % root] + list(extra)), verbose=False)


@pytest.fixture(scope="module")
def golden_tree(tmp_path_factory):
    from shapeclipper_amd.data import pix3d_mini
    root = str(tmp_path_factory.mktemp("g17") / "Pix3D")
    pix3d_mini.write_tree(root, n_per_cat=3, k_nearest=2, cat_key="chair,sofa", n_points=64)     # make_golden_pix3d.py's tree
    return root


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from shapeclipper_amd.data import pix3d_mini
    root = str(tmp_path_factory.mktemp("mini") / "Pix3D")
    pix3d_mini.write_tree(root, n_per_cat=6, k_nearest=5, cat_key="chair,sofa", n_points=256, seed=3)
    return root


def _flat(sample):
    out = {}
    for k, v in sample.items():
        if isinstance(v, dict):
            out.update({"%s.%s" % (k, kk): np.asarray(vv) for kk, vv in v.items()})
        else:
            out[k] = np.asarray(v)
    return out


@pytest.mark.parametrize("split", ["train", "test"])
def test_samples_are_bit_identical_to_the_reference_loader(golden, golden_tree, split):
    import data.pix3d as pix3d
    g = golden("g17_pix3d_loader")
    opt = _opt(golden_tree, ["--image_size=[32,32]", "--data.k_nearest=2", "--render.rand_sample=0"])
    ds = pix3d.Dataset(opt, split=split)
    assert ["%s/%s" % cn for cn in ds.list] == g["%s/list" % split].tolist()
    assert ds.label2cat == g["%s/label2cat" % split].tolist() == ["chair", "sofa"]
    idxs = sorted({int(k.split("/")[1]) for k in g.files if k.startswith(split + "/") and k.split("/")[1].isdigit()})
    assert idxs
    for i in idxs:
        got = _flat(ds[i])
        want = {k.split("/", 2)[2]: g[k] for k in g.files if k.startswith("%s/%d/" % (split, i))}
        assert sorted(got) == sorted(want), (split, i)
        for k in want:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (split, i, k)
            assert np.array_equal(got[k], want[k]), (split, i, k)
    out = os.path.join(os.path.dirname(golden_tree), "map_%s.txt" % split)
    ds.id_filename_mapping(opt, out)
    with open(out) as f:
        lines = [ln.replace(golden_tree, "data/Pix3D") for ln in f.read().splitlines()]
    assert lines == g["%s/id_filename_mapping" % split].tolist()


def test_the_dataset_keeps_its_own_copy_of_the_options(tree):
    import data.pix3d as pix3d
    opt = _opt(tree)
    ds = pix3d.Dataset(opt, split="test")
    opt.H, opt.W = opt.eval.image_size                           # what Runner.evaluate does
    s = ds[0]
    assert s["rgb_input_map"].shape == (3, 224, 224) and s["rgb_input"].shape == (224 * 224, 3) and "ray_idx" not in s
    assert "ray_seed" not in s                                   # the test split draws no rays (:235)


def test_default_root_and_the_clip_annotation_mode(tree):
    import data.pix3d as pix3d
    opt = _opt(tree)
    assert pix3d.Dataset(opt, split="train").path == tree
    opt.data.pix3d.pop("root")
    with pytest.raises(FileNotFoundError, match="data/Pix3D/lists/chair_train.txt"):
        pix3d.Dataset(opt, split="train")
    with pytest.raises(NotImplementedError, match="CLIP-annotation"):
        pix3d.Dataset(_opt(tree), split="train", transform=lambda x: x)


def test_ray_seeds_differ_per_sample_and_view():
    from shapeclipper_amd.data.pix3d import ray_seeds
    s = torch.stack([ray_seeds(123, i, 6) for i in range(50)])
    assert s.dtype == torch.int64 and s.shape == (50, 6)
    assert len(set(s.reshape(-1).tolist())) == 300
    assert torch.equal(ray_seeds(123, 7, 6), s[7]) and not torch.equal(ray_seeds(124, 7, 6), s[7])


@pytest.mark.parametrize("device_rays", [True, False])
def test_loader_collates_with_workers(tree, device_rays):
    import data.pix3d as pix3d
    R, K, B = 64, 5, 4
    opt = _opt(tree, ["--image_size=[48,48]", "--render.rand_sample=%d" % R, "--data.num_workers=2", "--batch_size=%d" % B]
               + ([] if device_rays else ["--hip.device_rays!"]))
    opt.world_size = 1
    ds = pix3d.Dataset(opt, split="train")
    batch = next(iter(ds.setup_loader(opt, shuffle=True)))
    assert batch["rgb_input_map"].shape == (B, 3, 48, 48) and batch["mask_input_map_NN"].shape == (B, 1, 48, 48, K)
    assert batch["pose_gt_NN"].shape == (B, 3, 4, K) and batch["dpc"]["points"].shape == (B, 256, 3)
    if device_rays:
        assert batch["ray_seed"].shape == (B, 1 + K) and batch["ray_seed"].dtype == torch.int64
        assert len(set(batch["ray_seed"].reshape(-1).tolist())) == B * (1 + K)
        assert "ray_idx" not in batch and "ray_idx_NN" not in batch and "rgb_input" not in batch
    else:
        assert "ray_seed" not in batch
        assert batch["ray_idx"].shape == (B, R) and batch["ray_idx"].dtype == torch.int64
        assert batch["ray_idx_NN"].shape == (B, R, K)
        assert batch["rgb_input"].shape == (B, R, 3) and batch["normal_input_NN"].shape == (B, R, 3, K)
        b, i = 1, 9
        p = int(batch["ray_idx"][b, i])
        assert torch.equal(batch["rgb_input"][b, i], batch["rgb_input_map"][b, :, p // 48, p % 48])
        for row in batch["ray_idx"]:
            assert len(set(row.tolist())) == R
