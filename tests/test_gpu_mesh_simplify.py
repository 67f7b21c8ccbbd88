"""ops.mesh_cluster_simplify (csrc/mesh_simplify.hip) on the GPU against the numpy restatement tests/mesh_simplify_ref.py, bit for bit:
the output vertices as uint32 views, the faces, the two maps and every count.  The kernel accumulates integers only (values rounded at
2^-24, 64-bit atomic adds) and solves in un-fused float64 in the header's order, so nothing less than equality is asked.

Shapes: the four marching-cubes meshes of a 17^3 grid (400 to 1,100 faces: several workgroups of the face passes) at pitch 2 and 3; the
sphere at 128 cells per axis (32,768 mask words: 128 rounds of the rank scan, faces spanning 8 cells whose terms saturate); the
hand-counted meshes of tests/mesh_topology_ref.py (4 to 32 faces, a degenerate face) and its 200-face soup (duplicate, opposite and
degenerate faces) in a 4-cell box; a batch with an empty image.  The restatement of every case is computed once and shared."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_simplify_ref as ref  # noqa: E402
import mesh_topology_ref as topo  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
_REF = {}


def _box4(verts):
    """The mesh rescaled into the box [0, 4]^3 (fp32): four cells of pitch 1 per axis."""
    v = np.asarray(verts, np.float32)
    lo, hi = v.min(), v.max()
    return ((v - lo) / (hi - lo) * np.float32(4.0)).astype(np.float32)


def _small():
    out = {name: (_box4(v), f) for name, (v, f, _) in topo.meshes().items()}
    sv, sf = topo.soup()
    out["soup"] = (_box4(sv), sf)
    return out


SMALL = _small()
SHAPE_CASES = [(name, pitch) for name in ("sphere", "torus", "cube", "plate") for pitch in (2, 3)]


def _case(key):
    """key -> (verts, faces, origin, pitch, cells): a marching-cubes shape at a pitch, or a small mesh in its 4-cell box."""
    if isinstance(key, tuple):
        name, pitch = key
        return (*ref.mc_mesh(name), (0.0, 0.0, 0.0), float(pitch), ref.cells_for(pitch))
    return (*SMALL[key], (0.0, 0.0, 0.0), 1.0, 4)


def _want(key, reg=0.05):
    if (key, reg) not in _REF:
        verts, faces, origin, pitch, cells = _case(key)
        _REF[(key, reg)] = ref.cluster_simplify(verts, faces, origin, pitch, cells, reg)
    return _REF[(key, reg)]


def _run(meshes, origin, pitch, cells, reg=0.05):
    """ops.mesh_cluster_simplify of a list of (verts, faces) numpy meshes packed into one batch."""
    from shapeclipper_amd import ops
    verts = torch.as_tensor(np.concatenate([np.asarray(v, np.float32).reshape(-1, 3) for v, _ in meshes])).to(DEV)
    faces = torch.as_tensor(np.concatenate([np.asarray(f, np.int32).reshape(-1, 3) for _, f in meshes])).to(DEV)
    v_count = torch.tensor([len(v) for v, _ in meshes], dtype=torch.int64)
    f_count = torch.tensor([len(f) for _, f in meshes], dtype=torch.int64)
    return ops.mesh_cluster_simplify(verts, faces, v_count, f_count, origin, pitch, cells, reg)


def _check(got, wants, v_in, what):
    """Image b of the result `got` equals the restatement wants[b], bit for bit."""
    assert got.verts.dtype == torch.float32 and got.faces.dtype == torch.int32 and got.vertex_cluster.dtype == torch.int32
    assert got.face_source.dtype == torch.int32 and got.v_count.dtype == torch.int64 and got.collapsed.dtype == torch.int64
    assert got.v_count.tolist() == [len(w["verts_out"]) for w in wants], (what, got.v_count.tolist())
    assert got.f_count.tolist() == [len(w["faces_out"]) for w in wants], (what, got.f_count.tolist())
    assert got.collapsed.tolist() == [w["collapsed"] for w in wants], (what, got.collapsed.tolist())
    assert got.cancelled.tolist() == [w["cancelled"] for w in wants], (what, got.cancelled.tolist())
    assert got.verts.shape[0] == int(got.v_count.sum()) and got.faces.shape[0] == int(got.f_count.sum()) == got.face_source.shape[0]
    verts, faces = got.verts.cpu().numpy(), got.faces.cpu().numpy()
    cluster, source = got.vertex_cluster.cpu().numpy(), got.face_source.cpu().numpy()
    v0 = f0 = i0 = 0
    for b, (want, n_in) in enumerate(zip(wants, v_in)):
        nv, nf = len(want["verts_out"]), len(want["faces_out"])
        mine = verts[v0:v0 + nv]
        differ = np.flatnonzero((mine.view(np.uint32) != want["verts_out"].view(np.uint32)).any(axis=1))
        assert differ.size == 0, (what, b, "verts_out", differ[:5], mine[differ[:5]], want["verts_out"][differ[:5]])
        assert np.array_equal(faces[f0:f0 + nf], want["faces_out"]), (what, b, "faces_out")
        assert np.array_equal(source[f0:f0 + nf], want["face_source"]), (what, b, "face_source")
        assert np.array_equal(cluster[i0:i0 + n_in], want["vertex_cluster"]), (what, b, "vertex_cluster")
        v0, f0, i0 = v0 + nv, f0 + nf, i0 + n_in
    assert i0 == cluster.shape[0]


def _bits(got):
    return [t.cpu().view(torch.int32 if t.dtype == torch.float32 else t.dtype).clone() for t in got]


@pytest.mark.parametrize("key", SHAPE_CASES, ids=lambda k: "%s-%d" % k)
def test_marching_cubes_shapes_at_pitch_two_and_three(key):
    verts, faces, origin, pitch, cells = _case(key)
    _check(_run([(verts, faces)], origin, pitch, cells), [_want(key)], [len(verts)], key)


@pytest.mark.parametrize("name", list(SMALL))
def test_small_meshes_in_a_four_cell_box(name):
    verts, faces, origin, pitch, cells = _case(name)
    got = _run([(verts, faces)], origin, pitch, cells)
    _check(got, [_want(name)], [len(verts)], name)
    if name == "soup":
        want = _want(name)
        print("soup: 200 faces -> %d, collapsed %d, cancelled %d" % (len(want["faces_out"]), want["collapsed"], want["cancelled"]))
        assert want["cancelled"] > 0 and 0 < len(want["faces_out"]) < 200 - want["cancelled"]      # degenerate faces take no part


def test_one_cell_per_axis_and_a_strong_pull():
    verts, faces = ref.mc_mesh("cube")
    got = _run([(verts, faces)], (0.0, 0.0, 0.0), 16.0, 1)
    _check(got, [ref.cluster_simplify(verts, faces, (0, 0, 0), 16.0, 1)], [len(verts)], "one cell")
    assert got.verts.shape == (1, 3) and got.faces.shape == (0, 3) and int(got.collapsed[0]) == len(faces)
    _check(_run([(verts, faces)], (0.0, 0.0, 0.0), 3.0, 6, reg=1.0), [_want(("cube", 3), 1.0)], [len(verts)], "reg 1")


def test_sphere_at_128_cells_per_axis_with_saturating_terms():
    verts, faces = ref.mc_mesh("sphere")
    args = ((-0.25, 0.125, 0.0), 0.12890625, 128)                            # the box [o, o + 16.5]: every vertex inside
    want = ref.cluster_simplify(verts, faces, *args)
    assert np.abs(want["acc"][:, 4:10]).max() >= 2 ** 36                       # a term met the clamp
    _check(_run([(verts, faces)], *args), [want], [len(verts)], "128 cells")


def test_a_batch_of_three_images_with_an_empty_one_in_the_middle():
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    a, b = ref.mc_mesh("torus"), ref.mc_mesh("plate")
    got = _run([a, empty, b], (0.0, 0.0, 0.0), 3.0, 6)
    nothing = dict(verts_out=np.zeros((0, 3), np.float32), faces_out=np.zeros((0, 3), np.int32), vertex_cluster=np.zeros(0, np.int32),
                   face_source=np.zeros(0, np.int32), collapsed=0, cancelled=0)
    _check(got, [_want(("torus", 3)), nothing, _want(("plate", 3))], [len(a[0]), 0, len(b[0])], "batch")
    only = _run([empty], (0.0, 0.0, 0.0), 3.0, 6)                            # no vertex and no face at all
    _check(only, [nothing], [0], "empty")


def test_vertices_exactly_on_the_upper_face_of_the_box_belong_to_the_last_cell():
    verts, faces = ref.mc_mesh("cube")
    verts = verts.copy()
    verts[verts[:, 0] > 12.0, 0] = 16.0                                       # the cube's +x side moves onto the box's face x = G h
    verts[5] = (16.0, 16.0, 16.0)
    want = ref.cluster_simplify(verts, faces, (0, 0, 0), 2.0, 8)
    assert want["vertex_cluster"][5] == len(want["verts_out"]) - 1
    _check(_run([(verts, faces)], (0.0, 0.0, 0.0), 2.0, 8), [want], [len(verts)], "upper face")


def test_a_vertex_that_is_not_finite_or_outside_the_box_raises():
    verts, faces = ref.mc_mesh("sphere")
    good = lambda: _check(_run([(verts, faces)], (0.0, 0.0, 0.0), 2.0, 8), [_want(("sphere", 2))], [len(verts)], "after a refusal")
    for value in (float("nan"), float("inf"), -0.001, 16.001):
        bad = verts.copy()
        bad[7, 1] = value
        with pytest.raises(ValueError, match="outside the box"):
            _run([(bad, faces)], (0.0, 0.0, 0.0), 2.0, 8)
    good()
    with pytest.raises(ValueError, match="outside the box"):                    # a batch: the second image's vertex
        bad = verts.copy()
        bad[-1, 2] = float("nan")
        _run([(verts, faces), (bad, faces)], (0.0, 0.0, 0.0), 2.0, 8)
    good()


def test_a_face_index_out_of_range_raises():
    verts, faces = ref.mc_mesh("sphere")
    for bad_index in (len(verts), -1, 2 ** 31 - 1):                            # flagged on the device, never dereferenced
        bad = faces.copy()
        bad[7, 1] = bad_index
        with pytest.raises(ValueError, match="vertex range"):
            _run([(verts, bad)], (0.0, 0.0, 0.0), 2.0, 8)
    with pytest.raises(ValueError, match="vertex range"):                       # 4 is in the batch's range, not in the second image's
        _run([(verts, faces), (SMALL["tetrahedron"][0], np.array([[4, 1, 2]], np.int32))], (0.0, 0.0, 0.0), 2.0, 8)
    _check(_run([(verts, faces)], (0.0, 0.0, 0.0), 2.0, 8), [_want(("sphere", 2))], [len(verts)], "after a refusal")


def test_alone_in_a_batch_and_on_a_side_stream_give_the_same_bits():
    torus, sphere = ref.mc_mesh("torus"), ref.mc_mesh("sphere")
    alone = _run([torus], (0.0, 0.0, 0.0), 2.0, 8)
    batch = _run([sphere, torus, sphere], (0.0, 0.0, 0.0), 2.0, 8)
    nv, nf = int(alone.v_count[0]), int(alone.f_count[0])
    v0, f0 = int(batch.v_count[0]), int(batch.f_count[0])
    assert batch.v_count.tolist()[1] == nv and batch.f_count.tolist()[1] == nf
    assert torch.equal(alone.verts.view(torch.int32), batch.verts[v0:v0 + nv].view(torch.int32))
    assert torch.equal(alone.faces, batch.faces[f0:f0 + nf]) and torch.equal(alone.face_source, batch.face_source[f0:f0 + nf])
    assert torch.equal(alone.vertex_cluster, batch.vertex_cluster[len(sphere[0]):len(sphere[0]) + len(torus[0])])
    assert int(alone.collapsed[0]) == int(batch.collapsed[1]) and int(alone.cancelled[0]) == int(batch.cancelled[1])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = _bits(_run([torus], (0.0, 0.0, 0.0), 2.0, 8))
    torch.cuda.synchronize()
    for a, b in zip(_bits(alone), other):
        assert torch.equal(a, b)


def test_two_consecutive_calls_and_a_permuted_face_list_give_the_same_bits():
    verts, faces = ref.mc_mesh("torus")
    first = _run([(verts, faces)], (0.0, 0.0, 0.0), 3.0, 6)
    second = _run([(verts, faces)], (0.0, 0.0, 0.0), 3.0, 6)
    for a, b in zip(_bits(first), _bits(second)):
        assert torch.equal(a, b)
    perm = np.random.RandomState(5).permutation(len(faces))
    third = _run([(verts, faces[perm])], (0.0, 0.0, 0.0), 3.0, 6)
    assert torch.equal(first.verts.view(torch.int32), third.verts.view(torch.int32))
    assert torch.equal(first.vertex_cluster, third.vertex_cluster) and torch.equal(first.collapsed, third.collapsed)
    _check(third, [ref.cluster_simplify(verts, faces[perm], (0, 0, 0), 3.0, 6)], [len(verts)], "permuted")


def test_refusals_before_any_launch_and_of_the_entry_point():
    from shapeclipper_amd import _lib, ops
    verts, faces = (torch.as_tensor(x).to(DEV) for x in ref.mc_mesh("sphere"))
    vc, fc = torch.tensor([verts.shape[0]]), torch.tensor([faces.shape[0]])
    call = lambda origin=(0.0, 0.0, 0.0), pitch=2.0, cells=8, reg=0.05, v=verts, f=faces, nv=vc, nf=fc: ops.mesh_cluster_simplify(
        v, f, nv, nf, origin, pitch, cells, reg)
    for kw in (dict(cells=0), dict(cells=129), dict(cells=8.0), dict(cells=True), dict(pitch=0.0), dict(pitch=-1.0), dict(pitch=float("nan")),
               dict(pitch=float("inf")), dict(pitch=1e-60), dict(reg=0.0), dict(reg=-0.05), dict(reg=float("nan")), dict(reg=float("inf")),
               dict(reg=True), dict(origin=(0.0, 0.0)), dict(origin=(0.0, float("nan"), 0.0)), dict(origin=None), dict(v=verts.double()),
               dict(f=faces.long()), dict(v=verts.cpu()), dict(f=faces.cpu()), dict(v=verts[:, :2]), dict(nv=torch.tensor([5])),
               dict(nf=torch.tensor([faces.shape[0], -1])), dict(nv=vc.float())):
        with pytest.raises(ValueError):
            call(**kw)
    lib = _lib.load()
    V, F = verts.shape[0], faces.shape[0]
    assert lib.sc_mesh_cluster_simplify_scratch_bytes(1, V, F, 8) > 0
    for sizes in ((1, V, F, 0), (1, V, F, 129), (0, V, F, 8), (65536, V, F, 8), (1, V, (1 << 26) + 1, 8), (1, -1, F, 8), (65535, V, F, 128)):
        assert lib.sc_mesh_cluster_simplify_scratch_bytes(*sizes) == 0, sizes
    off = torch.tensor([[0, V], [0, F]], dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.sc_mesh_cluster_simplify_scratch_bytes(1, V, F, 8) // 4 + 8, device=DEV)
    out_v, out_f = torch.empty(V, 3, device=DEV), torch.empty(F, 3, dtype=torch.int32, device=DEV)
    counts, vcl = torch.empty(4, 1, dtype=torch.int64, device=DEV), torch.empty(V, dtype=torch.int32, device=DEV)
    src, bad = torch.empty(F, dtype=torch.int32, device=DEV), torch.empty(2, dtype=torch.int32, device=DEV)
    p = _lib.ptr

    def entry(verts_=verts, cells=8, pitch=2.0, reg=0.05, scratch=ws.data_ptr(), counts_=counts, n_faces=F, origin_x=0.0):
        return lib.sc_mesh_cluster_simplify(p(verts_), p(faces), p(off[0]), p(off[1]), 1, V, n_faces, origin_x, 0.0, 0.0, pitch, cells, reg,
                                            scratch, p(out_v), p(out_f), p(counts_), p(vcl), p(src), p(bad[:1]), p(bad[1:]), _lib.stream())
    INVALID = 1                                                                 # hipErrorInvalidValue
    for kw in (dict(verts_=None), dict(counts_=None), dict(scratch=None), dict(scratch=ws.data_ptr() + 4), dict(cells=0), dict(cells=129),
               dict(pitch=0.0), dict(pitch=float("nan")), dict(reg=0.0), dict(reg=float("inf")), dict(n_faces=(1 << 26) + 1),
               dict(origin_x=float("inf"))):
        assert entry(**kw) == INVALID, kw
    assert entry() == 0
    torch.cuda.synchronize()
    assert bad.tolist() == [0, 0] and int(counts[1, 0]) == len(_want(("sphere", 2))["faces_out"])
    _check(call(), [_want(("sphere", 2))], [V], "after the refusals")
