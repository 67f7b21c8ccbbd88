#!/usr/bin/env python
"""Generate tests/golden/g17_pix3d_loader.npz from the REFERENCE's own data/pix3d.py (build container only).

The reference's data/pix3d.py, data/base.py, utils/util.py and utils/camera.py are imported unmodified and run on the miniature
tree of shapeclipper_amd/data/pix3d_mini.py (written into a temporary directory as data/Pix3D, the path the reference hard-codes).
Stubbed, because they are absent here: torchvision -- only `transforms.functional.to_tensor`, restated as torchvision does it for
8-bit images (uint8 HWC -> float32 CHW / 255) --, vigra (imported by utils/util.py, unused with render.rand_sample = 0) and
termcolor (log colours).  image_size 32x32, k_nearest 2; the train split with render.rand_sample = 0 (no ray sampling,
data/pix3d.py:235) and the test split.  Fixtures are data.

    python tests/golden/make_golden_pix3d.py
"""
import importlib
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
OUT = os.environ.get("GOLDEN_OUT", HERE)
H = W = 32
K = 2
N_PER_CAT = 3
SAMPLES = {"train": (5,), "test": (2,)}     # one sample per split (each with K neighbours), both named with the str.replace quirk

sys.path.insert(0, ROOT)
from shapeclipper_amd.data import pix3d_mini        # noqa: E402  (the build's fixture writer: data only)

sys.path.remove(ROOT)


def _to_tensor(pic):
    arr = np.array(pic, dtype=np.uint8)
    if arr.ndim == 2:
        arr = arr[:, :, None]
    return torch.from_numpy(arr).permute(2, 0, 1).contiguous().float().div(255)


tv = types.ModuleType("torchvision")
tv.transforms = types.ModuleType("torchvision.transforms")
tv.transforms.functional = types.ModuleType("torchvision.transforms.functional")
tv.transforms.functional.to_tensor = _to_tensor
sys.modules.update({"torchvision": tv, "torchvision.transforms": tv.transforms, "torchvision.transforms.functional": tv.transforms.functional})
for name in ("vigra", "termcolor"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["termcolor"].colored = lambda s, **k: s
for pkg in ("utils", "data"):
    for k in [k for k in sys.modules if k == pkg or k.startswith(pkg + ".")]:
        del sys.modules[k]
    m = types.ModuleType(pkg)
    m.__path__ = [os.path.join(REF, pkg)]
    sys.modules[pkg] = m
ref = importlib.import_module("data.pix3d")
assert os.path.realpath(ref.__file__).startswith(REF + os.sep)
from utils.util import EasyDict as edict            # noqa: E402  (reference's)


def options():
    return edict(H=H, W=W, image_size=[H, W], camera=edict(focal=4, dist=5), render=edict(rand_sample=0, ray_uniform_fac=5),
                 data=edict(dataset="pix3d", k_nearest=K, max_img_cat=None, num_workers=0, augment=None, bgcolor=1,
                            pix3d=edict(cat="chair,sofa")))


def flatten(sample, split):
    out = {}
    for k, v in sample.items():
        if isinstance(v, dict):
            for kk, vv in v.items():
                out["%s/%s.%s" % (split, k, kk)] = np.asarray(vv)
        else:
            out["%s/%s" % (split, k)] = np.asarray(v)
    return out


def main():
    arrays = {}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        pix3d_mini.write_tree(os.path.join(tmp, "data", "Pix3D"), n_per_cat=N_PER_CAT, k_nearest=K, cat_key="chair,sofa", n_points=64)
        os.chdir(tmp)
        try:
            for split, idxs in SAMPLES.items():
                ds = ref.Dataset(options(), split=split)
                for i in idxs:
                    arrays.update({k.replace(split + "/", "%s/%d/" % (split, i), 1): v for k, v in flatten(ds[i], split).items()})
                arrays["%s/list" % split] = np.array(["%s/%s" % cn for cn in ds.list])
                ds.id_filename_mapping(ds.opt, os.path.join(tmp, "map.txt"))
                with open(os.path.join(tmp, "map.txt")) as f:
                    arrays["%s/id_filename_mapping" % split] = np.array(f.read().replace(tmp + os.sep, "").splitlines())
                arrays["%s/label2cat" % split] = np.array(ds.label2cat)
        finally:
            os.chdir(cwd)
    path = os.path.join(OUT, "g17_pix3d_loader.npz")
    np.savez_compressed(path, **arrays)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(arrays), os.path.getsize(path)))


if __name__ == "__main__":
    main()
