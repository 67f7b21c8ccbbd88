"""ops.PackedMesh through every op that produces or consumes it (shapeclipper_amd/mesh_pack.py): both meshers return one, `*mesh` and
`*mesh.starts()` give each consumer the bits that hand-built arguments give it, and a SimplifiedMesh's `.packed` goes back in.  A
[3, 8, 8, 8] grid: a sphere, an image without a surface, an off-centre sphere."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S = 8
CENTRES = ((0.0, 0.0, 0.0), None, (0.2, -0.1, 0.1))
RADII = (0.6, None, 0.5)


def _level():
    ax = np.linspace(-1, 1, S)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    grids = [np.ones((S, S, S)) if c is None else np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r for c, r in zip(CENTRES, RADII)]
    return torch.tensor(np.stack(grids).astype(np.float32)).cuda()


def _same(a, b):
    a, b = (list(x) if isinstance(x, tuple) else [x] for x in (a, b))
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def _consumers_agree(mesh):
    from shapeclipper_amd import ops
    dev = mesh.verts.device
    assert isinstance(mesh, ops.PackedMesh) and isinstance(mesh, tuple) and len(mesh) == 4
    verts, faces, v_count, f_count = mesh
    assert v_count.dtype == f_count.dtype == torch.int64 and not v_count.is_cuda and not f_count.is_cuda
    assert v_count[1] == 0 and f_count[1] == 0 and v_count[0] > 0 and f_count[2] > 0
    # split() is slicing by the running sums
    v_end, f_end = np.cumsum(v_count.numpy()).tolist(), np.cumsum(f_count.numpy()).tolist()
    v_start, f_start = [0] + v_end[:-1], [0] + f_end[:-1]
    parts, doubled = mesh.split(), mesh.split(verts * 2)
    assert len(parts) == 3
    for b in range(3):
        assert torch.equal(parts[b][0], verts[v_start[b]:v_end[b]]) and torch.equal(parts[b][1], faces[f_start[b]:f_end[b]])
        assert torch.equal(doubled[b][0], verts[v_start[b]:v_end[b]] * 2) and torch.equal(doubled[b][1], parts[b][1])
    assert mesh.offsets().tolist() == [[0] + v_end, [0] + f_end]
    assert mesh.starts() == (v_start, f_start, f_count.tolist())
    # the counts spelling
    assert _same(tuple(ops.mesh_topology(*mesh)), tuple(ops.mesh_topology(verts, faces, v_count, f_count)))
    simple = ops.mesh_cluster_simplify(*mesh, (0.0, 0.0, 0.0), 1.0, S - 1)
    assert _same(tuple(simple), tuple(ops.mesh_cluster_simplify(verts, faces, v_count, f_count, (0.0, 0.0, 0.0), 1.0, S - 1)))
    assert isinstance(simple.packed, ops.PackedMesh) and all(x is y for x, y in zip(simple.packed, simple[:4]))
    assert simple.f_count[0] > 0 and simple.f_count[1] == 0 and simple.f_count[2] > 0
    assert _same(tuple(ops.mesh_topology(*simple.packed)), tuple(ops.mesh_topology(simple.verts, simple.faces, simple.v_count, simple.f_count)))
    points = (torch.rand(3, 33, 3, generator=torch.Generator().manual_seed(5)) * (S - 1)).to(dev)
    i32 = dict(dtype=torch.int32, device=dev)
    for m in (mesh, simple.packed):
        by_hand = ops.point_mesh_distance(points, m.verts, m.faces, torch.tensor(m.v_count.tolist(), **i32), torch.tensor(m.f_count.tolist(), **i32))
        assert _same(tuple(ops.point_mesh_distance(points, *m)), tuple(by_hand))
        assert torch.isinf(by_hand.dist2[1]).all() and torch.isfinite(by_hand.dist2[[0, 2]]).all()
    # the starts spelling
    A, _, rows = ops.texture_layout(int(f_count.max()), 4)
    assert _same(ops.texture_queries(verts, faces, *mesh.starts(), A, 4, -1.0, 1.0, S, rows),
                 ops.texture_queries(verts, faces, v_start, f_start, f_count.tolist(), A, 4, -1.0, 1.0, S, rows))
    pose = torch.tensor([[1.0, 0, 0, -3.5], [0, 1.0, 0, -3.5], [0, 0, 1.0, 10.0]], device=dev).expand(3, 1, 3, 4).contiguous()
    intr = torch.tensor([[40.0, 0, 16.0], [0, 40.0, 16.0], [0, 0, 1.0]], device=dev).expand(3, 3, 3).contiguous()
    drawn = ops.mesh_raster(verts, faces, *mesh.starts(), pose, intr, 32, 32, 0.05)
    assert _same(tuple(drawn), tuple(ops.mesh_raster(verts, faces, v_start, f_start, f_count.tolist(), pose, intr, 32, 32, 0.05)))
    assert (drawn.face[0] >= 0).any() and (drawn.face[1] == -1).all() and (drawn.face[2] >= 0).any()


def test_isosurface_mesh_is_a_packed_mesh_every_consumer_takes():
    from shapeclipper_amd import ops
    _consumers_agree(ops.isosurface_mesh(_level()))


def test_dual_contour_mesh_is_a_packed_mesh_every_consumer_takes():
    from shapeclipper_amd import ops
    level = _level()
    crossings = ops.isosurface_mesh(level)
    normals = []
    for (v, _), c in zip(crossings.split(), CENTRES):                  # unit normals: the sphere's gradient at the crossing vertices
        if c is not None:
            world = -1 + v * (2 / (S - 1))
            normals.append(torch.nn.functional.normalize(world - torch.tensor(c, device=v.device), dim=1))
    mesh = ops.dual_contour_mesh(level, torch.cat(normals).contiguous())
    _consumers_agree(mesh)
    empty = ops.dual_contour_mesh(level[1:2], torch.zeros(0, 3, device=level.device))
    assert isinstance(empty, ops.PackedMesh) and _same(tuple(empty), tuple(ops.PackedMesh.empty(1, level.device)))
    assert not empty.v_count.is_cuda and empty.verts.is_cuda
