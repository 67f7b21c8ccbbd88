"""PLY writers of the evaluation dumps (shapeclipper_amd/utils/util_vis.py; the reference's dump_meshes / dump_pointclouds_compare):
binary_little_endian 1.0, byte-exact headers, and a round trip through a small numpy reader.  CPU only."""
import os

import numpy as np
import pytest

from shapeclipper_amd.utils import util_vis
from shapeclipper_amd.utils.util import EasyDict as edict

MESH_HEADER = (b"ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
               b"element face %d\nproperty list uchar int vertex_indices\nend_header\n")
CLOUD_HEADER = (b"ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")


def read_ply(fname):
    """-> (header bytes, vertex records, face index array or None).  Faces are read one list at a time: no fixed count assumed."""
    data = open(fname, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header, body = data[:end], data[end:]
    lines = header.decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    counts, props, cur = {}, {}, None
    for l in lines[2:-1]:
        w = l.split()
        if w[0] == "element":
            cur = w[1]; counts[cur] = int(w[2]); props[cur] = []
        else:
            props[cur].append(w[1:])
    types = {"float": "<f4", "uchar": "u1", "int": "<i4"}
    vdt = np.dtype([(p[1], types[p[0]]) for p in props["vertex"]])
    verts = np.frombuffer(body, vdt, counts["vertex"])
    pos = vdt.itemsize * counts["vertex"]
    faces = None
    if "face" in counts:
        faces = []
        for _ in range(counts["face"]):
            n = body[pos]
            faces.append(np.frombuffer(body, "<i4", n, pos + 1))
            pos += 1 + 4 * n
        faces = np.asarray(faces, np.int32).reshape(-1, 3)
    assert pos == len(body)
    return header, verts, faces


def _opt(tmp_path):
    os.makedirs(tmp_path / "dump", exist_ok=True)
    return edict(output_path=str(tmp_path))


def test_mesh_round_trip_and_header(tmp_path):
    rng = np.random.RandomState(0)
    v = rng.randn(57, 3).astype(np.float32)
    f = rng.randint(0, 57, (101, 3)).astype(np.int32)
    util_vis.dump_meshes(_opt(tmp_path), [np.int64(7)], "mesh", [(v, f)])
    fname = tmp_path / "dump" / "7_mesh.ply"
    header, verts, faces = read_ply(fname)
    assert header == MESH_HEADER % (57, 101)
    assert np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], 1), v) and np.array_equal(faces, f)
    assert os.path.getsize(fname) == len(header) + 12 * 57 + 13 * 101


def test_empty_mesh_writes_no_file(tmp_path, capsys):
    opt = _opt(tmp_path)
    util_vis.dump_meshes(opt, [3, 4], "mesh", [(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)),
                                               (np.eye(3, dtype=np.float32), np.array([[0, 1, 2]], np.int32))])
    assert not (tmp_path / "dump" / "3_mesh.ply").exists() and (tmp_path / "dump" / "4_mesh.ply").exists()
    assert capsys.readouterr().out.strip().splitlines() == ["Mesh is empty!"]


def test_exportable_meshes_use_their_own_export(tmp_path):
    """The PyMCubes / trimesh branch hands over objects with .export (as the reference's dump_meshes uses them)."""
    seen = []

    class FakeMesh:
        def export(self, fname):
            seen.append(fname)

    util_vis.dump_meshes(_opt(tmp_path), [5], "mesh", [FakeMesh()])
    assert seen == ["{}/dump/5_mesh.ply".format(tmp_path)]


def test_pointcloud_compare_round_trip_and_colours(tmp_path):
    import torch
    rng = np.random.RandomState(1)
    pred, gt = rng.randn(2, 30, 3).astype(np.float32), rng.randn(2, 30, 3).astype(np.float32)
    util_vis.dump_pointclouds_compare(_opt(tmp_path), torch.tensor([11, 12]), "pointclouds_comp", torch.tensor(pred), torch.tensor(gt))
    for b, i in enumerate((11, 12)):
        header, verts, faces = read_ply(tmp_path / "dump" / ("%d_pointclouds_comp.ply" % i))
        assert header == CLOUD_HEADER % 60 and faces is None
        assert np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], 1), np.concatenate([pred[b], gt[b]]))
        rgb = np.stack([verts["red"], verts["green"], verts["blue"]], 1)
        assert (rgb[:30] == [255, 0, 0]).all() and (rgb[30:] == [0, 255, 0]).all()


def test_writers_take_arrays_of_any_float_and_int_type(tmp_path):
    v = np.arange(12, dtype=np.float64).reshape(4, 3) / 7
    f = np.array([[0, 1, 2], [1, 2, 3]], np.int64)
    util_vis.write_ply_mesh(str(tmp_path / "m.ply"), v, f)
    _, verts, faces = read_ply(tmp_path / "m.ply")
    assert np.array_equal(verts["y"], v[:, 1].astype(np.float32)) and np.array_equal(faces, f)
    with pytest.raises(Exception):
        util_vis.write_ply_mesh(str(tmp_path / "bad.ply"), v, np.zeros((2, 4), np.int32))
