"""A miniature Pix3D tree in the layout of the processed download (see data/pix3d.py), written from a seed.  The tests, the golden
generator (tests/golden/make_golden_pix3d.py) and tools/perf_silhouette_rays.py share it.

Source images are `size` (default 96x80, W x H), another size than the loader's target, so that the resize matters; masks have soft
edges (a linear ramp across the silhouette), so that the 0.5 threshold and Pillow's premultiplied RGBA resize matter.  One sample name
per category contains "img" and "mask", so that the reference's str.replace of every occurrence (data/pix3d.py:333-334) decides
where its files are."""
import csv
import json
import os

import numpy as np
import PIL.Image

CATEGORIES = ("chair", "sofa")


def sample_names(cat, n):
    return ["%s_%04d" % (cat, i) for i in range(n - 1)] + ["%s_img_mask_%d" % (cat, n - 1)]


def _rotation(rng):
    a, e, t = rng.uniform(-np.pi, np.pi), rng.uniform(-0.5, 0.5), rng.uniform(-0.2, 0.2)
    ca, sa, ce, se, ct, st = np.cos(a), np.sin(a), np.cos(e), np.sin(e), np.cos(t), np.sin(t)
    Ry = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]])
    Rx = np.array([[1, 0, 0], [0, ce, -se], [0, se, ce]])
    Rz = np.array([[ct, -st, 0], [st, ct, 0], [0, 0, 1]])
    return Rz @ Rx @ Ry


def _images(rng, W, H):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    cy, cx = H * rng.uniform(0.35, 0.65), W * rng.uniform(0.35, 0.65)
    ry, rx = H * rng.uniform(0.2, 0.4), W * rng.uniform(0.2, 0.4)
    r = np.sqrt(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2)
    ramp = rng.uniform(0.08, 0.25)                                  # soft edge width (in units of the radius)
    mask = np.clip((1 + ramp - r) / (2 * ramp), 0, 1)
    base = rng.uniform(0, 255, 3)
    grad = rng.uniform(-80, 80, (3, 2))
    rgb = base[None, None] + (yy[..., None] / H - 0.5) * grad[:, 0] + (xx[..., None] / W - 0.5) * grad[:, 1]
    rgb = rgb + rng.normal(0, 12, rgb.shape)
    normal = np.stack([(xx - cx) / rx, (yy - cy) / ry, np.ones_like(xx)], -1)
    normal = normal / np.linalg.norm(normal, axis=-1, keepdims=True) * 0.5 + 0.5 + rng.normal(0, 0.02, normal.shape)
    to8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    return to8(rgb), to8(mask * 255), to8(normal * 255)


def write_tree(root, n_per_cat=6, size=(96, 80), k_nearest=5, cat_key="chair,sofa", n_points=1000, seed=0,
               splits=("train", "test")):
    """Write the tree under root and return {split: [(cat, name)]}.  Both splits list every sample; CLIP_NN/{cat_key}_{split}.csv
    names k_nearest neighbours of each sample (other samples, in a seeded order); `cat_key` is the reference's CSV name for the
    category option (data/pix3d.py:97: opt.data.pix3d.cat with ", " replaced by "_")."""
    rng = np.random.RandomState(seed)
    W, H = size
    assert n_per_cat >= k_nearest + 1
    everything = []
    for cat in CATEGORIES:
        for name in sample_names(cat, n_per_cat):
            everything.append((cat, name))
            ann = dict(img="img/%s/%s.png" % (cat, name), mask="mask/%s/%s.png" % (cat, name),
                       model="model/%s/%s_model/model.obj" % (cat, name), focal_length=35.0,
                       cam_position=rng.uniform(-2, 2, 3).tolist(), rot_mat=_rotation(rng).tolist(),
                       trans_mat=rng.uniform(-0.1, 0.1, 3).tolist(), bbox=[4, 5, W - 6, H - 3])
            os.makedirs(os.path.join(root, "annotation", cat), exist_ok=True)
            with open(os.path.join(root, "annotation", cat, name + ".json"), "w") as f:
                json.dump(ann, f)
            rgb, mask, normal = _images(rng, W, H)
            img_path = ann["img"].replace("img", "img_processed")
            mask_path = ann["mask"].replace("mask", "mask_processed")
            normal_path = mask_path.replace("mask", "normal")
            for rel, arr in ((img_path, rgb), (mask_path, mask), (normal_path, normal)):
                os.makedirs(os.path.dirname(os.path.join(root, rel)), exist_ok=True)
                PIL.Image.fromarray(arr).save(os.path.join(root, rel))
            pc = os.path.join(root, "pointclouds", ann["model"][6:].replace(".obj", ".npy"))
            os.makedirs(os.path.dirname(pc), exist_ok=True)
            np.save(pc, rng.uniform(-0.4, 0.4, (n_points, 3)).astype(np.float32))
    os.makedirs(os.path.join(root, "lists"), exist_ok=True)
    os.makedirs(os.path.join(root, "CLIP_NN"), exist_ok=True)
    lists = {}
    for split in splits:
        lists[split] = everything
        for cat in CATEGORIES:
            with open(os.path.join(root, "lists", "%s_%s.txt" % (cat, split)), "w") as f:
                f.write("\n".join(n for c, n in everything if c == cat) + "\n")
        with open(os.path.join(root, "CLIP_NN", "%s_%s.csv" % (cat_key, split)), "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["query"] + ["nn%d" % i for i in range(k_nearest)])
            for i, (c, n) in enumerate(everything):
                others = [j for j in rng.permutation(len(everything)) if j != i][:k_nearest]
                w.writerow(["%s/%s.png" % (c, n)] + ["%s/%s.png" % everything[j] for j in others])
    return lists
