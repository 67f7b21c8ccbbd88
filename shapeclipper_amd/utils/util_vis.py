"""Evaluation dumps: PNG images (via PIL when available) and PLY geometry (numpy only) -- the reference's utils/util_vis.py
dump_images, dump_meshes and dump_pointclouds_compare.  Its TensorBoard grids and rotating GIFs are not reproduced."""
import os

import numpy as np
import torch

try:
    from PIL import Image
except Exception:  # pragma: no cover
    Image = None


@torch.no_grad()
def dump_images(opt, idx, name, images, masks=None, from_range=(0, 1), poses=None, folder="dump"):
    if Image is None:
        return
    lo, hi = from_range
    imgs = ((images - lo) / (hi - lo)).clamp(0, 1)
    if masks is not None:
        imgs = imgs * masks + (1 - masks)
    imgs = (imgs.cpu().permute(0, 2, 3, 1).numpy() * 255).astype(np.uint8)
    for i, img in zip(idx, imgs):
        arr = img[..., 0] if img.shape[-1] == 1 else img
        Image.fromarray(arr).save("{}/{}/{}_{}.png".format(opt.output_path, folder, int(i), name))


# ---- PLY (binary_little_endian 1.0): a header, then each element's rows as one packed structured array ----------------------------------
PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
PLY_FACE = np.dtype([("n", "u1"), ("vertex_indices", "<i4", (3,))])
PLY_COLOURED_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def _ply_header(n_vertices, n_faces=None, colours=False):
    lines = ["ply", "format binary_little_endian 1.0", "element vertex %d" % n_vertices,
             "property float x", "property float y", "property float z"]
    if colours:
        lines += ["property uchar red", "property uchar green", "property uchar blue"]
    if n_faces is not None:
        lines += ["element face %d" % n_faces, "property list uchar int vertex_indices"]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


def _numpy(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def write_ply_mesh(fname, vertices, faces):
    """vertices [V,3] float, faces [F,3] int (tensors or arrays) -> binary PLY with `element vertex` and `element face`."""
    v, f = _numpy(vertices).reshape(-1, 3), _numpy(faces).reshape(-1, 3)
    vert = np.empty(len(v), PLY_VERTEX)
    vert["x"], vert["y"], vert["z"] = v[:, 0], v[:, 1], v[:, 2]
    face = np.empty(len(f), PLY_FACE)
    face["n"], face["vertex_indices"] = 3, f
    with open(fname, "wb") as fh:
        fh.write(_ply_header(len(vert), len(face)) + vert.tobytes() + face.tobytes())


def write_ply_pointcloud(fname, points, colours):
    """points [N,3] float, colours [N,3] uint8 -> binary PLY with one `element vertex` of x y z red green blue."""
    p, c = _numpy(points).reshape(-1, 3), _numpy(colours).reshape(-1, 3)
    vert = np.empty(len(p), PLY_COLOURED_VERTEX)
    vert["x"], vert["y"], vert["z"] = p[:, 0], p[:, 1], p[:, 2]
    vert["red"], vert["green"], vert["blue"] = c[:, 0], c[:, 1], c[:, 2]
    with open(fname, "wb") as fh:
        fh.write(_ply_header(len(vert), colours=True) + vert.tobytes())


def dump_meshes(opt, idx, name, meshes, folder="dump"):
    """meshes: per sample a (vertices, faces) pair (eval_3D.meshes_device) or an object with .export (trimesh, when PyMCubes/trimesh are
    importable).  An empty mesh writes no file and prints one line, as the reference does."""
    for i, mesh in zip(idx, meshes):
        fname = "{}/{}/{}_{}.ply".format(opt.output_path, folder, int(i), name)
        if hasattr(mesh, "export"):
            try:
                mesh.export(fname)
            except Exception:
                print("Mesh is empty!")
            continue
        vertices, faces = mesh
        if len(faces) == 0:
            print("Mesh is empty!")
            continue
        write_ply_mesh(fname, vertices, faces)


def dump_pointclouds_compare(opt, idx, name, preds, gts, folder="dump"):
    """The prediction (red) and the ground truth (green) of every sample in one coloured point cloud."""
    for i in range(len(idx)):
        pred, gt = _numpy(preds[i]).reshape(-1, 3), _numpy(gts[i]).reshape(-1, 3)
        colours = np.zeros((len(pred) + len(gt), 3), np.uint8)
        colours[:len(pred), 0] = 255
        colours[len(pred):, 1] = 255
        fname = "{}/{}/{}_{}.ply".format(opt.output_path, folder, int(idx[i]), name)
        write_ply_pointcloud(fname, np.concatenate([pred, gt]), colours)
