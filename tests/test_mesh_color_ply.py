"""Coloured mesh PLYs (util_vis.write_ply_mesh with normals and colours, dump_meshes with eval_3D.mesh_attributes tuples) and the
`--hip.mesh_color` switch.  CPU only."""
import os

import numpy as np

from shapeclipper_amd.utils import util_vis
from shapeclipper_amd.utils.util import EasyDict as edict

FULL_HEADER = (b"ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
               b"property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
               b"element face %d\nproperty list uchar int vertex_indices\nend_header\n")


def read_mesh_ply(fname):
    """-> (header lines, vertex records with the header's own properties, faces [F,3])."""
    data = open(fname, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    n_v = int(lines[2].split()[2])
    types = {"float": "<f4", "uchar": "u1"}
    vdt = np.dtype([(l.split()[2], types[l.split()[1]]) for l in lines if l.startswith("property ") and "list" not in l])
    n_f = int([l for l in lines if l.startswith("element face")][0].split()[2])
    verts = np.frombuffer(data, vdt, n_v, end)
    rec = np.frombuffer(data, np.dtype([("n", "u1"), ("i", "<i4", (3,))]), n_f, end + vdt.itemsize * n_v)
    assert (rec["n"] == 3).all() and end + vdt.itemsize * n_v + 13 * n_f == len(data)
    return lines, verts, rec["i"]


def _mesh(seed, V=11, F=7):
    rng = np.random.RandomState(seed)
    v = rng.randn(V, 3).astype(np.float32)
    n = rng.randn(V, 3).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    c = rng.randint(0, 256, (V, 3)).astype(np.uint8)
    f = rng.randint(0, V, (F, 3)).astype(np.int32)
    return v, f, n, c


def test_header_and_round_trip(tmp_path):
    v, f, n, c = _mesh(0)
    fname = str(tmp_path / "m.ply")
    util_vis.write_ply_mesh(fname, v, f, normals=n, colours=c)
    data = open(fname, "rb").read()
    assert data.startswith(FULL_HEADER % (len(v), len(f)))
    lines, verts, faces = read_mesh_ply(fname)
    assert [l.split()[-1] for l in lines if l.startswith("property ") and "list" not in l] == \
        ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert verts.dtype.itemsize == 6 * 4 + 3                                         # packed records
    assert np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], 1), v)
    assert np.array_equal(np.stack([verts["nx"], verts["ny"], verts["nz"]], 1), n)
    assert np.array_equal(np.stack([verts["red"], verts["green"], verts["blue"]], 1), c)
    assert np.array_equal(faces, f)


def test_only_normals_or_only_colours(tmp_path):
    v, f, n, c = _mesh(1)
    for kw, props in ((dict(normals=n), ["x", "y", "z", "nx", "ny", "nz"]), (dict(colours=c), ["x", "y", "z", "red", "green", "blue"])):
        fname = str(tmp_path / "m.ply")
        util_vis.write_ply_mesh(fname, v, f, **kw)
        lines, verts, faces = read_mesh_ply(fname)
        assert list(verts.dtype.names) == props and np.array_equal(faces, f)


def test_without_attributes_the_bytes_are_unchanged(tmp_path):
    """The plain writer's bytes, stated independently: header, packed x y z records, then (uchar 3, int32 x 3) per face."""
    v, f, _, _ = _mesh(2)
    fname = str(tmp_path / "m.ply")
    util_vis.write_ply_mesh(fname, v, f)
    header = (b"ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              b"element face %d\nproperty list uchar int vertex_indices\nend_header\n") % (len(v), len(f))
    body = v.astype("<f4").tobytes() + b"".join(b"\x03" + row.astype("<i4").tobytes() for row in f)
    assert open(fname, "rb").read() == header + body
    util_vis.write_ply_mesh(str(tmp_path / "n.ply"), v, f, normals=None, colours=None)
    assert open(str(tmp_path / "n.ply"), "rb").read() == header + body


def test_dump_meshes_takes_attribute_tuples(tmp_path, capsys):
    os.makedirs(tmp_path / "dump")
    opt = edict(output_path=str(tmp_path))
    v, f, n, c = _mesh(3)
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
    util_vis.dump_meshes(opt, [4, 9], "mesh_color", [(v, f, n, c), empty])
    assert sorted(os.listdir(tmp_path / "dump")) == ["4_mesh_color.ply"]           # the empty mesh writes no file ...
    assert "Mesh is empty!" in capsys.readouterr().out                             # ... and prints its line
    _, verts, faces = read_mesh_ply(str(tmp_path / "dump" / "4_mesh_color.ply"))
    assert np.array_equal(np.stack([verts["red"], verts["green"], verts["blue"]], 1), c) and np.array_equal(faces, f)
    # a plain (vertices, faces) pair still writes the plain file
    util_vis.dump_meshes(opt, [5], "mesh", [(v, f)])
    lines, _, _ = read_mesh_ply(str(tmp_path / "dump" / "5_mesh.ply"))
    assert "property float nx" not in lines and "property uchar red" not in lines


def test_switch_defaults_off():
    from shapeclipper_amd.model import runner
    from shapeclipper_amd.utils import options
    assert options.HIP_DEFAULTS["hip"]["mesh_color"] is False
    opt = options.set(options.parse_arguments(["--yaml=options/pix3d/config.yaml", "--name=pytest_mc", "--output_root=/tmp/sc_pytest"]),
                      verbose=False)
    assert opt.hip.mesh_color is False and not runner._mesh_color(opt)
    opt = options.set(options.parse_arguments(["--yaml=options/pix3d/config.yaml", "--name=pytest_mc", "--output_root=/tmp/sc_pytest",
                                               "--hip.mesh_color"]), verbose=False)
    assert runner._mesh_color(opt)
