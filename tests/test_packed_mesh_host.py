"""shapeclipper_amd/mesh_pack.py on the host: PackedMesh's methods against literal values, and every refusal of the two checkers that needs
no device, with its exception class."""
import pytest
import torch

from shapeclipper_amd import mesh_pack
from shapeclipper_amd.mesh_pack import PackedMesh, check_counts, check_packed, check_starts

I32 = torch.int32


def _mesh(v_count, f_count):
    """Vertex k of the packed array is (k, 10 k, 100 k); face k of the packed array is (k, k, k)."""
    V, F = sum(v_count), sum(f_count)
    verts = torch.arange(V, dtype=torch.float32)[:, None] * torch.tensor([1.0, 10.0, 100.0])
    faces = torch.arange(F, dtype=I32)[:, None].expand(F, 3).contiguous()
    return PackedMesh(verts, faces, torch.tensor(v_count, dtype=torch.int64), torch.tensor(f_count, dtype=torch.int64))


def _rows(t):
    return t[:, 0].tolist()


def test_mesh_pack_is_pure_torch():
    imports = [line for line in open(mesh_pack.__file__).read().splitlines() if line.startswith(("import ", "from "))]
    assert imports == ["import collections", "import torch"]            # neither the library nor ops: it runs on a CPU


def test_three_images_with_an_empty_middle_one():
    m = _mesh([4, 0, 3], [2, 0, 1])
    verts, faces, v_count, f_count = m                                  # a plain 4-tuple to whoever unpacks it
    assert verts is m.verts and f_count is m.f_count and len(m) == 4 and isinstance(m, tuple)
    off = m.offsets()
    assert off.dtype == torch.int64 and off.device.type == "cpu" and off.tolist() == [[0, 4, 4, 7], [0, 2, 2, 3]]
    assert m.starts() == ([0, 4, 4], [0, 2, 2], [2, 0, 1])
    assert all(type(x) is int for s in m.starts() for x in s)
    parts = m.split()
    assert [(_rows(v), _rows(f)) for v, f in parts] == [([0.0, 1.0, 2.0, 3.0], [0, 1]), ([], []), ([4.0, 5.0, 6.0], [2])]
    assert parts[1][0].shape == (0, 3) and parts[1][1].shape == (0, 3) and parts[2][1].dtype == I32
    other = torch.arange(7)[:, None] * torch.tensor([[2, 3]])           # another per-vertex tensor of V rows
    parts = m.split(other)
    assert [(_rows(v), _rows(f)) for v, f in parts] == [([0, 2, 4, 6], [0, 1]), ([], []), ([8, 10, 12], [2])]
    assert parts[0][0].shape == (4, 2)
    P, rows = m.padded_rows(1)
    assert P == 4 and rows.dtype == torch.int64 and rows.tolist() == [[0, 1, 2, 3], [4, 4, 4, 4], [4, 5, 6, 4]]
    P, rows = m.padded_rows(16)
    assert P == 16 and rows.tolist() == [list(range(4)) + [0] * 12, [4] * 16, [4, 5, 6] + [4] * 13]
    assert m.padded_rows()[0] == 4 and torch.equal(m.padded_rows()[1], m.padded_rows(1)[1])      # multiple = 1 by default


def test_an_empty_last_image_starts_at_the_clamped_row():
    m = _mesh([2, 0], [1, 0])
    assert m.padded_rows(1)[1].tolist() == [[0, 1], [1, 1]]             # the start 2 = V is clamped to V - 1
    assert m.padded_rows(4)[1].tolist() == [[0, 1, 0, 0], [1, 1, 1, 1]]


def test_one_image_and_int32_counts():
    m = _mesh([3], [2])
    m = m._replace(v_count=m.v_count.to(I32), f_count=m.f_count.to(I32))
    assert isinstance(m, PackedMesh)
    assert m.offsets().dtype == torch.int64 and m.offsets().tolist() == [[0, 3], [0, 2]]
    assert m.starts() == ([0], [0], [2])
    (v, f), = m.split()
    assert torch.equal(v, m.verts) and torch.equal(f, m.faces)
    assert m.padded_rows(1)[1].tolist() == [[0, 1, 2]]
    P, rows = m.padded_rows(16)
    assert P == 16 and rows.tolist() == [[0, 1, 2] + [0] * 13]
    m17 = _mesh([17], [0])
    assert m17.padded_rows(16)[0] == 32 and m17.padded_rows(1)[0] == 17 and _mesh([16], [0]).padded_rows(16)[0] == 16


def test_no_image_and_no_vertex():
    m = _mesh([], [])
    assert m.offsets().tolist() == [[0], [0]] and m.starts() == ([], [], []) and m.split() == [] and m.padded_rows(16) == (0, None)
    m = _mesh([0, 0], [0, 0])
    assert m.padded_rows(1) == (0, None) and m.padded_rows(16) == (0, None)
    assert [(tuple(v.shape), tuple(f.shape)) for v, f in m.split()] == [((0, 3), (0, 3))] * 2


@pytest.mark.parametrize("B", [0, 1, 3])
def test_empty_round_trips(B):
    m = PackedMesh.empty(B, torch.device("cpu"))
    assert isinstance(m, PackedMesh) and m.verts.shape == (0, 3) and m.verts.dtype == torch.float32
    assert m.faces.shape == (0, 3) and m.faces.dtype == I32
    for c in (m.v_count, m.f_count):
        assert c.dtype == torch.int64 and c.device.type == "cpu" and c.tolist() == [0] * B
    assert m.offsets().tolist() == [[0] * (B + 1)] * 2
    assert m.starts() == ([0] * B, [0] * B, [0] * B)
    assert [(tuple(v.shape), tuple(f.shape)) for v, f in m.split()] == [((0, 3), (0, 3))] * B
    assert m.padded_rows(1) == (0, None) and m.padded_rows(16) == (0, None)
    counts, offsets = check_counts("t", m.v_count, m.f_count, 0, 0)
    assert counts.shape == (2, B) and torch.equal(offsets, m.offsets())
    assert check_starts("t", *m.starts(), 0, 0, 65535) == m.starts()


def test_ops_reexports_the_type():
    from shapeclipper_amd import ops
    assert ops.PackedMesh is PackedMesh and ops.check_packed is check_packed and ops.check_starts is check_starts
    s = ops.SimplifiedMesh(*range(8))
    assert len(s) == 8 and isinstance(s.packed, PackedMesh) and tuple(s.packed) == (0, 1, 2, 3)
    assert list(s._asdict()) == ["verts", "faces", "v_count", "f_count", "vertex_cluster", "face_source", "collapsed", "cancelled"]


# ---- the checkers ------------------------------------------------------------------------------------------------------------------------
def test_check_counts():
    m = _mesh([4, 0, 3], [2, 0, 1])
    counts, offsets = check_counts("who", m.v_count, m.f_count, 7, 3)
    assert counts.dtype == torch.int64 and counts.tolist() == [[4, 0, 3], [2, 0, 1]] and torch.equal(offsets, m.offsets())
    counts, _ = check_counts("who", m.v_count.to(I32), m.f_count.to(I32), 7, 3)
    assert counts.dtype == torch.int64
    for v_count, f_count, V, F in (([4, -1, 4], [2, 0, 1], 7, 3),      # a negative count whose sum is right
                                   ([4, 0, 3], [3, -1, 1], 7, 3),
                                   ([4, 0, 3], [2, 0, 1], 8, 3), ([4, 0, 3], [2, 0, 1], 6, 3),     # a vertex sum off by one
                                   ([4, 0, 3], [2, 0, 1], 7, 4), ([4, 0, 3], [2, 0, 1], 7, 2),     # a face sum off by one
                                   ([], [], 1, 0), ([], [], 0, 1)):
        with pytest.raises(ValueError, match="who: v_count / f_count must be non-negative and sum to the packed lengths"):
            check_counts("who", torch.tensor(v_count, dtype=torch.int64), torch.tensor(f_count, dtype=torch.int64), V, F)


def test_check_packed_refusals_up_to_the_device_check():
    m = _mesh([4, 0, 3], [2, 0, 1])
    kw = dict(max_images=65535, max_faces=1 << 26)
    for bad, name in ((dict(verts=[[0.0, 0.0, 0.0]]), "verts must be a tensor"), (dict(faces=None), "faces must be a tensor"),
                      (dict(v_count=[4, 0, 3]), "v_count must be a tensor"), (dict(f_count=(2, 0, 1)), "f_count must be a tensor"),
                      (dict(verts=m.verts.double()), "verts must be torch.float32"), (dict(faces=m.faces.long()), "faces must be torch.int32"),
                      (dict(v_count=m.v_count.float()), "v_count must be torch.int64 or torch.int32"),
                      (dict(f_count=m.f_count.to(torch.int16)), "f_count must be torch.int64 or torch.int32"),
                      (dict(verts=m.verts[:, :2]), r"verts must be \[n,3\]"), (dict(faces=m.faces[:, :2]), r"faces must be \[n,3\]"),
                      (dict(faces=m.faces.view(-1)), r"faces must be \[n,3\]"),
                      (dict(f_count=m.f_count[:2]), "v_count and f_count"), (dict(v_count=m.v_count[None]), "v_count and f_count"),
                      ({}, "verts is a CPU tensor")):                   # the device check itself: nothing before it objects to m
        with pytest.raises(ValueError, match="who: " + name):
            check_packed("who", *m._replace(**bad), **kw)


def test_check_starts():
    assert check_starts("who", [0, 4, 4], [0, 2, 2], [2, 0, 1], 7, 3, 65535) == ([0, 4, 4], [0, 2, 2], [2, 0, 1])
    got = check_starts("who", torch.tensor([0, 4]), (0, 2), [torch.tensor(2), 1.0], 7, 3, 2)     # anything int() takes
    assert got == ([0, 4], [0, 2], [2, 1]) and all(type(x) is int for s in got for x in s)
    assert check_starts("who", [7], [3], [0], 7, 3, 1) == ([7], [3], [0])                        # an empty image at the very end
    for bad in (([0], [0, 2], [2, 1]), ([0, 4], [0], [2, 1]), ([0, 4], [0, 2], [2]), ([], [], [1]),       # unequal lengths
                ([0, 4, 4], [0, 2, 2], [2, 0, 1], 7, 3, 2),                                               # more images than max_images
                ([0, 4], [0, 2], [2, -1]),                                                                 # a negative f_count
                ([0, 4], [0, 2], [2, 2]), ([0, 4], [0, 4], [2, 0]),                                        # f_start + f_count > F
                ([0, 4], [-1, 2], [2, 1]),
                ([0, 8], [0, 2], [2, 1]), ([-1, 4], [0, 2], [2, 1])):                                      # v_start > V, < 0
        args = bad if len(bad) == 6 else bad + (7, 3, 65535)
        with pytest.raises(ValueError, match="who"):
            check_starts("who", *args)
    with pytest.raises(ValueError, match="image 1's faces .* outside the 3 faces / 7 vertices"):
        check_starts("who", [0, 4], [0, 2], [2, 2], 7, 3, 65535)
    with pytest.raises(ValueError, match="one length <= 2"):
        check_starts("who", [0, 0, 0], [0, 0, 0], [0, 0, 0], 7, 3, 2)


def test_the_ops_refuse_host_meshes_by_these_checks():
    """Without a device: the refusals of the four consumers that come before anything is loaded or launched."""
    from shapeclipper_amd import ops
    m = _mesh([4, 0, 3], [2, 0, 1])
    with pytest.raises(ValueError, match="mesh_topology: verts is a CPU tensor"):
        ops.mesh_topology(*m)
    with pytest.raises(ValueError, match="mesh_cluster_simplify: v_count and f_count"):
        ops.mesh_cluster_simplify(m.verts, m.faces, m.v_count, m.f_count[:1], (0.0, 0.0, 0.0), 1.0, 8)
    with pytest.raises(ValueError, match="mesh_raster: verts must be a device tensor"):
        ops.mesh_raster(m.verts, m.faces, *m.starts(), None, None, 8, 8, 0.05)
    with pytest.raises(ValueError, match="texture_queries: verts must be a device tensor"):
        ops.texture_queries(m.verts, m.faces, *m.starts(), 64, 8, -0.5, 0.5, 16, 8)
    with pytest.raises(ValueError, match="point_mesh_distance: points is a CPU tensor"):
        ops.point_mesh_distance(torch.zeros(3, 5, 3), *m)
