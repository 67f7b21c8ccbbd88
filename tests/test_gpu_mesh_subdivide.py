"""ops.mesh_subdivide and ops.mesh_project_step (csrc/mesh_subdivide.hip) on the GPU against the numpy restatement
tests/mesh_subdivide_ref.py, bit for bit: the output vertices as uint32 views, the faces, the fixed mask and the counts.  The kernel decides
everything by integer atomics, sorts every neighbour row and runs un-fused float64 in the header's order, so nothing less than equality
is asked.

Shapes: the marching-cubes meshes of a 17^3 grid (sphere, torus, cube) and a sphere that the grid face cuts open (400 to 1,100 faces) at
levels 1 and 2 (up to 4,352 faces into the second level: several workgroups and several rounds of the scans); the hand meshes of the host
test; a closed double cone whose two apexes have 300 neighbours (the rows a whole wave ranks); a batch with an empty image.  The
restatement of every case is computed once and shared."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_subdivide_ref as ref  # noqa: E402
import mesh_topology_ref as topo  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SHAPES = ("sphere", "torus", "cube", "cut_sphere")
HAND = {
    "octahedron": (ref.OCTA_V, ref.OCTA_F),
    "tetrahedron": (topo.TET_V, topo.TET_F),
    "unit cube": (topo.CUBE_V, topo.CUBE_F),
    "triangle": (np.array([[0, 0, 0], [2, 0, 0], [0, 4, 6]], np.float32), np.array([[0, 1, 2]], np.int32)),
    "three faces on an edge": (np.array([[0, 0, 0], [0, 0, 2], [1, 0, 1], [-1, 1, 1], [-1, -1, 1]], np.float32),
                               np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]], np.int32)),
    "doubled pair": (np.array([[0, 0, 0], [8, 0, 0], [0, 8, 0]], np.float32), np.array([[0, 1, 2], [0, 2, 1]], np.int32)),
    "same face twice": (np.array([[0, 0, 0], [8, 0, 0], [0, 8, 0], [5, 5, 5]], np.float32), np.array([[0, 1, 2], [0, 1, 2]], np.int32)),
}
_REF = {}


def _mesh(name):
    if name in HAND:
        return HAND[name]
    if name == "small torus":
        return topo.torus()
    return ref.double_cone() if name == "cone" else ref.shape(name)


def _want(name, levels=1):
    if (name, levels) not in _REF:
        _REF[(name, levels)] = ref.mesh_subdivide(*_mesh(name)) if levels == 1 else ref.mesh_subdivide(
            _want(name, levels - 1)["verts"], _want(name, levels - 1)["faces"])
    return _REF[(name, levels)]


def _run(meshes, levels=1, table_slots=None):
    """ops.mesh_subdivide of a list of (verts, faces) numpy meshes packed into one batch."""
    from shapeclipper_amd import ops
    verts = torch.as_tensor(np.concatenate([np.asarray(v, np.float32).reshape(-1, 3) for v, _ in meshes])).to(DEV)
    faces = torch.as_tensor(np.concatenate([np.asarray(f, np.int32).reshape(-1, 3) for _, f in meshes])).to(DEV)
    v_count = torch.tensor([len(v) for v, _ in meshes], dtype=torch.int64)
    f_count = torch.tensor([len(f) for _, f in meshes], dtype=torch.int64)
    return ops.mesh_subdivide(verts, faces, v_count, f_count, levels, table_slots)


def _bits(got):
    """The tensors of a SubdividedMesh as integer views on the host: equal lists mean equal bits."""
    view = {torch.float32: torch.int32, torch.bool: torch.uint8}
    return [t.cpu().view(view.get(t.dtype, t.dtype)).clone() for t in got]


def _check(got, wants, what):
    """Image b of the result `got` equals the restatement wants[b], bit for bit."""
    B = len(wants)
    assert got.verts.dtype == torch.float32 and got.faces.dtype == torch.int32 and got.fixed.dtype == torch.bool
    assert got.verts.is_cuda and got.faces.is_cuda and got.fixed.is_cuda and not got.v_count.is_cuda and not got.f_count.is_cuda
    assert all(getattr(got, k).dtype == torch.int64 and getattr(got, k).shape == (B,) for k in ("v_count", "f_count", "edges", "sharp_edges",
                                                                                              "fixed_vertices"))
    assert got.v_count.tolist() == [w["vertices_out"] for w in wants] and got.f_count.tolist() == [len(w["faces"]) for w in wants]
    assert got.verts.shape == (int(got.v_count.sum()), 3) and got.faces.shape == (int(got.f_count.sum()), 3)
    assert got.fixed.shape == (got.verts.shape[0],)
    assert got.packed.verts is got.verts and got.packed.faces is got.faces and got.packed.v_count is got.v_count
    verts, faces, fixed = got.verts.cpu().numpy(), got.faces.cpu().numpy(), got.fixed.cpu().numpy()
    v0 = f0 = 0
    for b, want in enumerate(wants):
        nv, nf = want["vertices_out"], len(want["faces"])
        mine = verts[v0:v0 + nv]
        differ = np.flatnonzero((mine.view(np.uint32) != want["verts"].view(np.uint32)).any(axis=1))
        assert differ.size == 0, (what, b, "verts", differ[:5], mine[differ[:5]], want["verts"][differ[:5]])
        assert np.array_equal(faces[f0:f0 + nf], want["faces"]), (what, b, "faces")
        assert np.array_equal(fixed[v0:v0 + nv], want["fixed"]), (what, b, "fixed")
        for k in ("edges", "sharp_edges", "fixed_vertices"):
            assert int(getattr(got, k)[b]) == want[k], (what, b, k, int(getattr(got, k)[b]), want[k])
        v0, f0 = v0 + nv, f0 + nf


@pytest.mark.parametrize("levels", (1, 2))
@pytest.mark.parametrize("name", SHAPES)
def test_marching_cubes_shapes(name, levels):
    want = _want(name, levels)
    _check(_run([_mesh(name)], levels), [want], (name, levels))
    assert len(want["faces"]) == 4 ** levels * len(_mesh(name)[1])
    if name == "cut_sphere":
        assert want["sharp_edges"] > 0 and want["fixed_vertices"] > want["sharp_edges"]


@pytest.mark.parametrize("name", tuple(HAND) + ("small torus",))
def test_hand_meshes(name):
    for levels in (1, 2, 3):
        _check(_run([_mesh(name)], levels), [_want(name, levels)], (name, levels))


def test_a_hub_of_300_spokes_is_ranked_by_a_wave():
    want = _want("cone")
    assert want["degree_max"] == 300 and want["sharp_edges"] == 0
    _check(_run([_mesh("cone")]), [want], "cone")
    _check(_run([_mesh("cone")], 2), [_want("cone", 2)], "cone, two levels")


def test_a_batch_of_three_images_with_an_empty_one_in_the_middle():
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    nothing = dict(verts=np.zeros((0, 3), np.float32), faces=np.zeros((0, 3), np.int32), fixed=np.zeros(0, bool), vertices_out=0, edges=0,
                   sharp_edges=0, fixed_vertices=0)
    for levels in (1, 2):
        batch = _run([_mesh("cut_sphere"), empty, _mesh("torus")], levels)
        _check(batch, [_want("cut_sphere", levels), nothing, _want("torus", levels)], ("batch", levels))
    _check(_run([empty]), [nothing], "no vertex and no face at all")
    _check(_run([empty, _mesh("octahedron"), empty, empty]), [nothing, _want("octahedron"), nothing, nothing], "empty images around one")
    points = np.arange(12, dtype=np.float32).reshape(4, 3)                              # vertices without a face stay where they are
    only = _run([(points, empty[1])], 2)
    assert torch.equal(only.verts.cpu(), torch.as_tensor(points)) and only.v_count.tolist() == [4] and only.f_count.tolist() == [0]
    assert only.edges.tolist() == [0] and not only.fixed.any()
    extra = (np.concatenate([ref.OCTA_V, points]), ref.OCTA_F)                          # isolated vertices between the old and the new ones
    _check(_run([extra, extra]), [ref.mesh_subdivide(*extra)] * 2, "isolated vertices")


def test_table_size_second_run_and_side_stream_change_no_bit():
    verts, faces = _mesh("cut_sphere")
    first = _bits(_run([(verts, faces)], 2))
    slots = 1 << (3 * len(faces)).bit_length()                                          # the smallest table: long probe chains
    assert slots > 3 * len(faces)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        on_side = _bits(_run([(verts, faces)], 2))
    torch.cuda.synchronize()
    for what, other in (("second run", _bits(_run([(verts, faces)], 2))), ("small table", _bits(_run([(verts, faces)], 2, table_slots=slots))),
                        ("large table", _bits(_run([(verts, faces)], 2, table_slots=64 * slots))), ("side stream", on_side)):
        assert len(first) == len(other) == 8
        for a, b in zip(first, other):
            assert torch.equal(a, b), what


def test_permuted_faces_permute_the_output_and_change_no_position():
    verts, faces = _mesh("cut_sphere")
    perm = np.random.RandomState(5).permutation(len(faces))
    moved = (verts, np.roll(faces[perm], 1, axis=1))
    got = _run([moved])
    _check(got, [ref.mesh_subdivide(*moved)], "permuted faces")
    key = lambda v: sorted(map(tuple, np.ascontiguousarray(v).view(np.uint32).tolist()))
    assert key(got.verts.cpu().numpy()) == key(_want("cut_sphere")["verts"])


def test_the_three_device_flags_raise():
    verts, faces = _mesh("sphere")
    for value in (float("nan"), float("inf"), -float("inf")):
        bad = verts.copy()
        bad[7, 1] = value
        with pytest.raises(ValueError, match="a vertex is not finite"):
            _run([(bad, faces)])
    with pytest.raises(ValueError, match="a vertex is not finite"):                     # a batch: the second image's last vertex
        bad = verts.copy()
        bad[-1, 2] = float("nan")
        _run([(verts, faces), (bad, faces)], 2)
    for bad_index in (len(verts), -1, 2 ** 31 - 1):                                     # flagged on the device, never dereferenced
        bad = faces.copy()
        bad[7, 1] = bad_index
        with pytest.raises(ValueError, match="vertex range"):
            _run([(verts, bad)])
    with pytest.raises(ValueError, match="vertex range"):                               # 4 is in the batch's range, not in the second image's
        _run([(verts, faces), (topo.TET_V, np.array([[4, 1, 2]], np.int32))])
    for corners in ((0, 1), (1, 2), (2, 0)):
        bad = faces.copy()
        bad[11, corners[1]] = bad[11, corners[0]]
        with pytest.raises(ValueError, match="a face repeats a vertex index"):
            _run([(verts, bad)])
    _check(_run([(verts, faces)]), [_want("sphere")], "after the refusals")


def test_refusals_before_any_launch_and_of_the_entry_point(monkeypatch):
    from shapeclipper_amd import _lib, ops
    verts, faces = (torch.as_tensor(x).to(DEV) for x in _mesh("sphere"))
    V, F = verts.shape[0], faces.shape[0]
    vc, fc = torch.tensor([V]), torch.tensor([F])
    call = lambda levels=1, slots=None, v=verts, f=faces, nv=vc, nf=fc: ops.mesh_subdivide(v, f, nv, nf, levels, slots)
    step = lambda v=verts, s=None, g=None, fx=None, scale=1.0, max_step=0.5: ops.mesh_project_step(
        v, torch.zeros(V, device=DEV) if s is None else s, torch.ones(V, 3, device=DEV) if g is None else g,
        torch.zeros(V, dtype=torch.bool, device=DEV) if fx is None else fx, scale, max_step)
    lib = _lib.load()
    launched = []

    def no_launch():
        launched.append(1)
        raise AssertionError("the library was asked for before the arguments were refused")

    monkeypatch.setattr(_lib, "load", no_launch)
    for kw, name in ((dict(levels=0), "levels"), (dict(levels=4), "levels"), (dict(levels=1.0), "levels"), (dict(levels=True), "levels"),
                     (dict(levels=None), "levels"), (dict(slots=3 * F), "table_slots"), (dict(slots=(1 << (3 * F).bit_length()) + 2), "table_slots"),
                     (dict(slots=1 << 31), "table_slots"), (dict(slots=4096.0), "table_slots"), (dict(v=verts.double()), "verts"),
                     (dict(f=faces.long()), "faces"), (dict(v=verts.cpu()), "verts"), (dict(f=faces.cpu()), "faces"), (dict(v=verts[:, :2]), "verts"),
                     (dict(nv=torch.tensor([5])), "v_count"), (dict(nf=torch.tensor([F, -1])), "v_count"), (dict(nv=vc.float()), "v_count")):
        with pytest.raises(ValueError, match=name):
            call(**kw)
    for kw, name in ((dict(v=verts.cpu()), "verts"), (dict(v=verts.double()), "verts"), (dict(s=torch.zeros(V + 1, device=DEV)), "sdf"),
                     (dict(g=torch.ones(V, 2, device=DEV)), "grad"), (dict(fx=torch.zeros(V, dtype=torch.uint8, device=DEV)), "fixed"),
                     (dict(scale=0.0), "scale"), (dict(scale=float("nan")), "scale"), (dict(scale=True), "scale"), (dict(max_step=-1.0), "max_step"),
                     (dict(max_step=float("inf")), "max_step"), (dict(max_step="0.5"), "max_step")):
        with pytest.raises(ValueError, match=name):
            step(**kw)
    # an empty batch launches nothing: the library is not even loaded
    none = ops.mesh_subdivide(verts[:0], faces[:0], torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 2)
    assert none.verts.shape == (0, 3) and none.faces.shape == (0, 3) and none.fixed.shape == (0,) and none.edges.shape == (0,)
    assert ops.mesh_project_step(verts[:0], torch.zeros(0, device=DEV), verts[:0], torch.zeros(0, dtype=torch.bool, device=DEV), 1.0, 0.5).shape == (0, 3)
    assert not launched
    monkeypatch.undo()
    T = ops.mesh_topology_slots(F)
    assert lib.sc_mesh_subdivide_scratch_bytes(1, V, F, T) > 0 and lib.sc_mesh_subdivide_scratch_bytes(3, 0, 0, 2) > 0
    for sizes in ((1, V, F, 0), (1, V, F, T + 2), (1, V, F, 512), (0, V, F, T), (65536, V, F, T), (1, V, (1 << 24) + 1, 1 << 30), (1, -1, F, T),
                  (1, (1 << 30) + 1, F, T)):
        assert lib.sc_mesh_subdivide_scratch_bytes(*sizes) == 0, sizes
    off = torch.tensor([[0, V], [0, F]], dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.sc_mesh_subdivide_scratch_bytes(1, V, F, T) // 4 + 8, device=DEV)
    out_v, out_f = torch.empty(V + 3 * F, 3, device=DEV), torch.empty(4 * F, 3, dtype=torch.int32, device=DEV)
    out_x = torch.empty(V + 3 * F, dtype=torch.bool, device=DEV)
    counts = torch.empty(6, 1, dtype=torch.int64, device=DEV)
    bad = torch.empty(3, dtype=torch.int32, device=DEV)
    p = _lib.ptr

    def entry(verts_=verts, slots=T, scratch=ws.data_ptr(), counts_=counts, n_faces=F, out=out_v, faces_out=out_f, fixed_out=out_x, n_images=1):
        return lib.sc_mesh_subdivide(p(verts_), p(faces), p(off[0]), p(off[1]), n_images, V, n_faces, slots, scratch, p(out), p(faces_out),
                                     p(fixed_out), p(counts_), p(bad[:1]), p(bad[1:2]), p(bad[2:]), _lib.stream())
    INVALID = 1                                                                         # hipErrorInvalidValue
    for kw in (dict(verts_=None), dict(out=None), dict(faces_out=None), dict(fixed_out=None), dict(counts_=None), dict(scratch=None),
               dict(scratch=ws.data_ptr() + 4), dict(slots=512), dict(slots=T + 2), dict(n_faces=(1 << 24) + 1), dict(n_images=65536)):
        assert entry(**kw) == INVALID, kw
    assert entry(n_images=0) == 0
    assert lib.sc_mesh_project_step(None, None, None, None, 0, 1.0, 0.5, None, _lib.stream()) == 0
    assert lib.sc_mesh_project_step(None, None, None, None, 5, 1.0, 0.5, None, _lib.stream()) == INVALID
    assert lib.sc_mesh_project_step(p(verts), p(verts), p(verts), p(out_x), -1, 1.0, 0.5, p(out_v), _lib.stream()) == INVALID
    assert entry() == 0
    torch.cuda.synchronize()
    want = _want("sphere")
    assert bad.tolist() == [0, 0, 0] and counts[:, 0].tolist() == [want[k] for k in ref.INTS]
    n = want["vertices_out"]
    assert torch.equal(out_v[:n].cpu().view(torch.int32), torch.as_tensor(want["verts"]).view(torch.int32))
    assert torch.equal(out_f.cpu(), torch.as_tensor(want["faces"])) and torch.equal(out_x[:n].cpu(), torch.as_tensor(want["fixed"]))
    _check(call(), [want], "after the refusals")
    # all six counts of a shape with a rim, isolated vertices and a hub, through the entry point's rows
    cone_v, cone_f = ref.double_cone()
    for name, (v_, f_) in (("cut_sphere", _mesh("cut_sphere")), ("cone and points", (np.concatenate([cone_v, cone_v[:3] + 9]), cone_f))):
        w = ref.mesh_subdivide(v_, f_)
        got = _run([(v_, f_)])
        assert [got.v_count[0].item(), got.edges[0].item(), got.sharp_edges[0].item(), got.fixed_vertices[0].item()] == [w[k] for k in ref.INTS[:4]]
        tv, tf = torch.as_tensor(v_).to(DEV), torch.as_tensor(f_).to(DEV)
        o = torch.tensor([[0, len(v_)], [0, len(f_)]], dtype=torch.int64, device=DEV)
        slots = ops.mesh_topology_slots(len(f_))
        ws2 = torch.empty(lib.sc_mesh_subdivide_scratch_bytes(1, len(v_), len(f_), slots) // 4 + 8, device=DEV)
        ov, of_ = torch.empty(len(v_) + 3 * len(f_), 3, device=DEV), torch.empty(4 * len(f_), 3, dtype=torch.int32, device=DEV)
        ox = torch.empty(len(v_) + 3 * len(f_), dtype=torch.bool, device=DEV)
        assert lib.sc_mesh_subdivide(p(tv), p(tf), p(o[0]), p(o[1]), 1, len(v_), len(f_), slots, p(ws2), p(ov), p(of_), p(ox), p(counts),
                                     p(bad[:1]), p(bad[1:2]), p(bad[2:]), _lib.stream()) == 0
        torch.cuda.synchronize()
        assert counts[:, 0].tolist() == [w[k] for k in ref.INTS], name


def test_project_step_bit_for_bit():
    from shapeclipper_amd import ops
    rng = np.random.RandomState(12)
    n = 1000
    verts = rng.uniform(0, 16, (n, 3)).astype(np.float32)
    sdf = rng.normal(0, 0.05, n).astype(np.float32)
    grad = (rng.normal(0, 1, (n, 3)) * rng.uniform(0.2, 3.0, (n, 1))).astype(np.float32)
    fixed = rng.uniform(size=n) < 0.1
    grad[0:20] = 0.0                                                                    # zero gradient
    grad[20:30] *= np.float32(1e-8)                                                     # g2 about 1e-16 < 1e-12
    grad[30:40] *= np.float32(1e-6)                                                     # g2 about 1e-12: either side of the threshold
    sdf[40:50] = np.nan
    sdf[50:55] = np.inf
    grad[55:60, 1] = np.inf
    grad[60:65, 2] = np.nan
    sdf[65:100] *= np.float32(40.0)                                                     # steps longer than max_step
    sdf[100:105], grad[100:105] = np.float32(1e30), np.float32(1e-5)                    # the step's length overflows
    grad[105:110] = np.float32(3e19)                                                    # g2 overflows
    sdf[110:120] = 0.0
    for scale, max_step in ((63.0 / 1.2, 0.5), (1.0, 0.5), (7.25, 0.0), (0.1, 1e9)):
        want = ref.project_step(verts, sdf, grad, fixed, scale, max_step)
        got = ops.mesh_project_step(*(torch.as_tensor(x).to(DEV) for x in (verts, sdf, grad, fixed)), scale, max_step)
        assert got.dtype == torch.float32 and got.shape == (n, 3)
        differ = np.flatnonzero((got.cpu().numpy().view(np.uint32) != want.view(np.uint32)).any(axis=1))
        assert differ.size == 0, (scale, max_step, differ[:5], got.cpu().numpy()[differ[:5]], want[differ[:5]])
        kept = (got.cpu().numpy().view(np.uint32) == verts.view(np.uint32)).all(axis=1)
        assert kept[fixed].all() and kept[:30].all() and kept[40:65].all() and kept[100:110].all()
        if max_step == 0.5 and scale > 1:
            step = np.sqrt(((got.cpu().numpy().astype(np.float64) - verts) ** 2).sum(axis=1))
            assert (~kept).sum() > 700 and step.max() <= 0.5 + 1e-5 and (step > 0.499).sum() >= 20     # the clamp is active
