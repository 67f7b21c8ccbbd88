"""Evaluation and training-time dumps: PNG images with optional pose axes and rotating GIFs (via PIL when available), PLY geometry
(numpy only) and textured Wavefront OBJ meshes -- the reference's utils/util_vis.py dump_images, draw_pose, dump_gifs, dump_meshes and
dump_pointclouds_compare; the OBJ / MTL writers have no counterpart there.  The GIF frames arrive as bytes (ops.vis_frames computes the
reference's float -> uint8 recipe on the device).  Its TensorBoard grids are not
reproduced."""
import os

import numpy as np
import torch

try:
    from PIL import Image, ImageDraw
except Exception:  # pragma: no cover
    Image = ImageDraw = None


@torch.no_grad()
def dump_images(opt, idx, name, images, masks=None, from_range=(0, 1), poses=None, folder="dump"):
    """{idx}_{name}.png per image of [B,C,H,W] in from_range; masks composite on white.  poses [B,3,4]: the axes of each rotation drawn in
    the top-left corner (draw_pose, size 20, width 2) on the 8-bit image, which is then saved as RGB."""
    if Image is None:
        return
    lo, hi = from_range
    imgs = ((images - lo) / (hi - lo)).clamp(0, 1)
    if masks is not None:
        imgs = imgs * masks + (1 - masks)
    imgs = (imgs.cpu().permute(0, 2, 3, 1).numpy() * 255).astype(np.uint8)
    rots = poses[..., :3].detach().cpu() if poses is not None else None
    for k, (i, img) in enumerate(zip(idx, imgs)):
        arr = img[..., 0] if img.shape[-1] == 1 else img
        image = Image.fromarray(arr)
        if rots is not None:
            image = draw_pose(image, rots[k], size=20, width=2).convert("RGB")
        image.save("{}/{}/{}_{}.png".format(opt.output_path, folder, int(i), name))


def dump_arrays(opt, idx, name, arrays, folder="dump"):
    """{idx}_{name}.npy per sample: arrays [B, ...] (tensor or numpy) saved as they are, one numpy file each (raw per-pixel quantities a PNG
    would quantise, e.g. the depth map of the surface render)."""
    for i, a in zip(idx, _numpy(arrays)):
        np.save("{}/{}/{}_{}.npy".format(opt.output_path, folder, int(i), name), a)


def dump_lines(opt, idx, name, lines, folder="dump"):
    """{idx}_{name}.txt per sample: one line of text each (a sidecar of a per-sample file, written by the rank that has the sample)."""
    for i, line in zip(idx, lines):
        with open("{}/{}/{}_{}.txt".format(opt.output_path, folder, int(i), name), "w") as f:
            f.write(line + "\n")


def draw_pose(image, rot, size=15, width=1):
    """The reference's draw_pose on an 8-bit PIL image: the first two coordinates of each column of rot [3,3] (the rotated x, y, z axes) as
    red, green and blue lines from (size, size), drawn on a transparent layer and alpha-composited.  -> RGBA image.  (The reference goes
    float -> mul(255).byte() -> PIL and back through to_tensor; the 8-bit image it draws on is the one dump_images makes.)"""
    base = image.convert("RGBA")
    layer = Image.new("RGBA", base.size, (0, 0, 0, 0))
    draw = ImageDraw.Draw(layer)
    center = (size, size)
    endpoint = [(float(size + size * p[0]), float(size + size * p[1])) for p in rot.t()]
    draw.line([center, endpoint[0]], fill=(255, 0, 0), width=width)
    draw.line([center, endpoint[1]], fill=(0, 255, 0), width=width)
    draw.line([center, endpoint[2]], fill=(0, 0, 255), width=width)
    base.alpha_composite(layer)
    return base


def dump_gifs(opt, idx, name, frames, folder="dump"):
    """frames: uint8 [B, V, H, W, 3] (ops.vis_frames) -> per sample {idx}_{name}.gif of its V frames, 100 ms each, looping forever
    (reference dump_gifs: PIL, convert('RGB'), save_all)."""
    if Image is None:
        return
    frames = _numpy(frames)
    for i, clip in zip(idx, frames):
        images = [Image.fromarray(f).convert("RGB") for f in clip]
        fname = "{}/{}/{}_{}.gif".format(opt.output_path, folder, int(i), name)
        images[0].save(fname, format="GIF", append_images=images[1:], save_all=True, duration=100, loop=0)


# ---- PLY (binary_little_endian 1.0): a header, then each element's rows as one packed structured array ----------------------------------
PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
PLY_FACE = np.dtype([("n", "u1"), ("vertex_indices", "<i4", (3,))])
PLY_COLOURED_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def _ply_header(n_vertices, n_faces=None, colours=False, normals=False):
    lines = ["ply", "format binary_little_endian 1.0", "element vertex %d" % n_vertices,
             "property float x", "property float y", "property float z"]
    if normals:
        lines += ["property float nx", "property float ny", "property float nz"]
    if colours:
        lines += ["property uchar red", "property uchar green", "property uchar blue"]
    if n_faces is not None:
        lines += ["element face %d" % n_faces, "property list uchar int vertex_indices"]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


def _numpy(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def write_ply_mesh(fname, vertices, faces, normals=None, colours=None):
    """vertices [V,3] float, faces [F,3] int (tensors or arrays) -> binary PLY with `element vertex` and `element face`.  The vertex
    element is x y z, then nx ny nz (float) when normals [V,3] are given, then red green blue (uchar) when colours [V,3] uint8 are."""
    v, f = _numpy(vertices).reshape(-1, 3), _numpy(faces).reshape(-1, 3)
    fields = list(PLY_VERTEX.descr)
    if normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if colours is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    vert = np.empty(len(v), np.dtype(fields))
    vert["x"], vert["y"], vert["z"] = v[:, 0], v[:, 1], v[:, 2]
    if normals is not None:
        n = _numpy(normals).reshape(-1, 3)
        vert["nx"], vert["ny"], vert["nz"] = n[:, 0], n[:, 1], n[:, 2]
    if colours is not None:
        c = _numpy(colours).reshape(-1, 3)
        vert["red"], vert["green"], vert["blue"] = c[:, 0], c[:, 1], c[:, 2]
    face = np.empty(len(f), PLY_FACE)
    face["n"], face["vertex_indices"] = 3, f
    with open(fname, "wb") as fh:
        fh.write(_ply_header(len(vert), len(face), colours=colours is not None, normals=normals is not None) + vert.tobytes() + face.tobytes())


def write_ply_pointcloud(fname, points, colours, normals=None):
    """points [N,3] float, colours [N,3] uint8 -> binary PLY with one `element vertex` of x y z red green blue; with normals [N,3] float
    the element is x y z nx ny nz red green blue (write_ply_mesh's order)."""
    p, c = _numpy(points).reshape(-1, 3), _numpy(colours).reshape(-1, 3)
    if normals is None:
        vert = np.empty(len(p), PLY_COLOURED_VERTEX)
    else:
        vert = np.empty(len(p), np.dtype(PLY_VERTEX.descr + [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")] + PLY_COLOURED_VERTEX.descr[3:]))
        n = _numpy(normals).reshape(-1, 3)
        vert["nx"], vert["ny"], vert["nz"] = n[:, 0], n[:, 1], n[:, 2]
    vert["x"], vert["y"], vert["z"] = p[:, 0], p[:, 1], p[:, 2]
    vert["red"], vert["green"], vert["blue"] = c[:, 0], c[:, 1], c[:, 2]
    with open(fname, "wb") as fh:
        fh.write(_ply_header(len(vert), colours=True, normals=normals is not None) + vert.tobytes())


def dump_meshes(opt, idx, name, meshes, folder="dump"):
    """meshes: per sample a (vertices, faces) pair (eval_3D.meshes_device), a (vertices, faces, normals, colours) tuple
    (eval_3D.mesh_attributes) or an object with .export (trimesh, when PyMCubes/trimesh are importable).  An empty mesh writes no file and
    prints one line, as the reference does."""
    for i, mesh in zip(idx, meshes):
        fname = "{}/{}/{}_{}.ply".format(opt.output_path, folder, int(i), name)
        if hasattr(mesh, "export"):
            try:
                mesh.export(fname)
            except Exception:
                print("Mesh is empty!")
            continue
        vertices, faces, *attributes = mesh
        if len(faces) == 0:
            print("Mesh is empty!")
            continue
        write_ply_mesh(fname, vertices, faces, *attributes)


def dump_pointclouds_compare(opt, idx, name, preds, gts, folder="dump", pred_normals=None, gt_normals=None):
    """The prediction (red) and the ground truth (green) of every sample in one coloured point cloud; with both clouds' normals [B,N,3]
    the vertices carry nx ny nz as well."""
    for i in range(len(idx)):
        pred, gt = _numpy(preds[i]).reshape(-1, 3), _numpy(gts[i]).reshape(-1, 3)
        colours = np.zeros((len(pred) + len(gt), 3), np.uint8)
        colours[:len(pred), 0] = 255
        colours[len(pred):, 1] = 255
        fname = "{}/{}/{}_{}.ply".format(opt.output_path, folder, int(idx[i]), name)
        normals = None
        if pred_normals is not None:
            normals = np.concatenate([_numpy(pred_normals[i]).reshape(-1, 3), _numpy(gt_normals[i]).reshape(-1, 3)])
        write_ply_pointcloud(fname, np.concatenate([pred, gt]), colours, normals)


# ---- textured Wavefront OBJ: {name}.obj + {name}.mtl + {name}.png (`--eval.texture`, eval_3D.mesh_texture) ---------------------------
def write_obj_textured(fname, vertices, faces, uv, mtl_name):
    """vertices [V,3] float, faces [F,3] int, uv [F,3,2] float (a texture coordinate per face corner: every face has its own chart) ->
    ASCII OBJ: `mtllib` with the bare file name of mtl_name, the V `v` lines, 3 F `vt` lines in face order, `usemtl tex` and the F faces
    as `f a/ta b/tb c/tc`, all indices 1-based.  Nine significant digits: an fp32 value reads back to the same bits."""
    v, f = _numpy(vertices).reshape(-1, 3), _numpy(faces).reshape(-1, 3)
    t = _numpy(uv).reshape(-1, 2)
    assert len(t) == 3 * len(f), "one texture coordinate per face corner"
    lines = ["mtllib %s" % os.path.basename(mtl_name)]
    lines += ["v %.9g %.9g %.9g" % (float(p[0]), float(p[1]), float(p[2])) for p in v]
    lines += ["vt %.9g %.9g" % (float(p[0]), float(p[1])) for p in t]
    lines.append("usemtl tex")
    lines += ["f %d/%d %d/%d %d/%d" % (a[0] + 1, 3 * k + 1, a[1] + 1, 3 * k + 2, a[2] + 1, 3 * k + 3) for k, a in enumerate(f.tolist())]
    with open(fname, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def write_mtl(fname, png_name):
    """The material `tex` of write_obj_textured: white ambient and diffuse, the diffuse map `map_Kd` naming png_name's bare file name (it
    lies beside the .mtl)."""
    with open(fname, "w") as fh:
        fh.write("newmtl tex\nKa 1 1 1\nKd 1 1 1\nmap_Kd %s\n" % os.path.basename(png_name))


_WARNED_NO_PIL = []


def dump_textured_meshes(opt, idx, name, meshes, folder="dump"):
    """meshes: per sample an eval_3D.TexturedMesh -> {idx}_{name}.obj, {idx}_{name}.mtl, {idx}_{name}.png (the colour atlas, the MTL's
    map_Kd) and {idx}_{name}_normal.png (the object-space normal atlas).  An empty mesh writes an OBJ without faces and its grey atlases.
    Without PIL there is no texture to point at: nothing is written, with one warning per process."""
    if Image is None:
        if not _WARNED_NO_PIL:
            _WARNED_NO_PIL.append(True)
            print("warning: PIL is not importable -- the textured OBJ dump ({idx}_%s.*) is skipped" % name)
        return
    for i, mesh in zip(idx, meshes):
        base = "{}/{}/{}_{}".format(opt.output_path, folder, int(i), name)
        write_obj_textured(base + ".obj", mesh.vertices, mesh.faces, mesh.uv, base + ".mtl")
        write_mtl(base + ".mtl", base + ".png")
        Image.fromarray(_numpy(mesh.atlas)).save(base + ".png")
        Image.fromarray(_numpy(mesh.normal_atlas)).save(base + "_normal.png")


def dump_atlases(opt, idx, name, atlases, folder="dump"):
    """{idx}_{name}.png per sample of a uint8 atlas [A,A] (grey) or [A,A,3] each, the bytes as they are (sizes may differ from sample to
    sample): a further map in the layout of {idx}_mesh_tex.png, e.g. the ambient occlusion of `--mesh.ao`."""
    if Image is None:
        return
    for i, atlas in zip(idx, atlases):
        Image.fromarray(_numpy(atlas)).save("{}/{}/{}_{}.png".format(opt.output_path, folder, int(i), name))
