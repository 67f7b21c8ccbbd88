"""ops.mesh_smooth (csrc/mesh_smooth.hip) on the GPU against the numpy restatement tests/mesh_smooth_ref.py, bit for bit: the output
vertices as uint32 views, the four integers and the four float64 measures as int64 views.  The kernel decides everything by integer
atomics, sorts every neighbour row and runs un-fused float64 in the header's order, so nothing less than equality is asked.

Shapes: the four marching-cubes meshes of a 17^3 grid and a sphere that the grid face cuts open (400 to 1,100 faces, 200 to 600 vertices:
several workgroups and several chunks of the sums) at 1, 2 and 10 iterations, Taubin and plain Laplacian; the hand-counted tetrahedron,
cube and torus of tests/mesh_topology_ref.py and its 200-face soup (non-manifold edges, duplicate and degenerate faces, 11 neighbours a
vertex); a closed double cone whose two apexes have 300 neighbours (the rows a whole wave ranks); a batch with an empty image.  The
restatement of every case is computed once and shared."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_smooth_ref as ref  # noqa: E402
import mesh_topology_ref as topo  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SHAPES = ("sphere", "torus", "cube", "plate", "cut_sphere")
SMALL = ("tetrahedron", "cube", "torus", "soup")
_REF = {}


def _mesh(name):
    """A 17^3 shape by name, a small mesh as ("small", name), the double cone as "cone"."""
    if isinstance(name, tuple):
        if name[1] == "soup":
            return topo.soup()
        return topo.meshes()[name[1]][:2]
    return ref.double_cone() if name == "cone" else ref.shape(name)


def _want(name, iters, lam=ref.LAM, mu=ref.MU):
    key = (name, iters, lam, mu)
    if key not in _REF:
        _REF[key] = ref.mesh_smooth(*_mesh(name), iters, lam, mu)
    return _REF[key]


def _run(meshes, iters, lam=ref.LAM, mu=ref.MU, table_slots=None):
    """ops.mesh_smooth of a list of (verts, faces) numpy meshes packed into one batch."""
    from shapeclipper_amd import ops
    verts = torch.as_tensor(np.concatenate([np.asarray(v, np.float32).reshape(-1, 3) for v, _ in meshes])).to(DEV)
    faces = torch.as_tensor(np.concatenate([np.asarray(f, np.int32).reshape(-1, 3) for _, f in meshes])).to(DEV)
    v_count = torch.tensor([len(v) for v, _ in meshes], dtype=torch.int64)
    f_count = torch.tensor([len(f) for _, f in meshes], dtype=torch.int64)
    return ops.mesh_smooth(verts, faces, v_count, f_count, iters, lam, mu, table_slots)


def _bits(got):
    """The tensors of a SmoothedMesh as integer views on the host: equal lists mean equal bits."""
    view = {torch.float32: torch.int32, torch.float64: torch.int64}
    return [t.cpu().view(view.get(t.dtype, t.dtype)).clone() for t in got]


def _check(got, wants, what):
    """Image b of the result `got` equals the restatement wants[b], bit for bit."""
    assert got.verts.dtype == torch.float32 and got.faces.dtype == torch.int32
    assert all(getattr(got, k).dtype == torch.int64 and getattr(got, k).shape == (len(wants),) and getattr(got, k).is_cuda for k in ref.INTS)
    assert all(getattr(got, k).dtype == torch.float64 and getattr(got, k).shape == (len(wants),) and getattr(got, k).is_cuda
               for k in ref.MEASURES)
    assert got.v_count.tolist() == [len(w["verts"]) for w in wants] and got.verts.shape[0] == int(got.v_count.sum())
    assert got.packed.verts is got.verts and got.packed.faces is got.faces
    verts = got.verts.cpu().numpy()
    v0 = 0
    for b, want in enumerate(wants):
        nv = len(want["verts"])
        mine = verts[v0:v0 + nv]
        differ = np.flatnonzero((mine.view(np.uint32) != want["verts"].view(np.uint32)).any(axis=1))
        assert differ.size == 0, (what, b, "verts", differ[:5], mine[differ[:5]], want["verts"][differ[:5]])
        for k in ref.INTS:
            assert int(getattr(got, k)[b]) == want[k], (what, b, k, int(getattr(got, k)[b]), want[k])
        for k in ref.MEASURES:
            mine_k = np.float64(float(getattr(got, k)[b]))
            assert mine_k.view(np.int64) == np.float64(want[k]).view(np.int64), (what, b, k, repr(mine_k), repr(want[k]))
        v0 += nv


@pytest.mark.parametrize("mu", (ref.MU, 0.0), ids=("taubin", "laplacian"))
@pytest.mark.parametrize("iters", (1, 2, 10))
@pytest.mark.parametrize("name", SHAPES)
def test_marching_cubes_shapes(name, iters, mu):
    want = _want(name, iters, mu=mu)
    _check(_run([_mesh(name)], iters, mu=mu), [want], (name, iters, mu))
    if name == "cut_sphere":
        assert want["fixed_boundary"] > 0
    if iters == 10 and mu != 0.0:
        print("%s: %d vertices, %d free, degree_max %d, roughness %.6f -> %.6f, displacement mean %.6f max %.6f"
              % (name, len(want["verts"]), want["free"], want["degree_max"], want["rough_before"], want["rough_after"], want["disp_mean"],
                 want["disp_max"]))


@pytest.mark.parametrize("name", SMALL)
def test_small_meshes_and_the_soup(name):
    key = ("small", name)
    for iters, lam, mu in ((1, 1.0, 0.0), (3, ref.LAM, ref.MU)):
        _check(_run([_mesh(key)], iters, lam, mu), [_want(key, iters, lam, mu)], (name, iters))
    if name == "soup":
        want = _want(key, 3, ref.LAM, ref.MU)
        verts, faces = _mesh(key)
        assert want["degree_max"] == len(verts) - 1 and max(ref.edge_counts(faces, len(verts)).values()) >= 3       # non-manifold edges


def test_no_iteration_returns_the_input_bits():
    verts, faces = _mesh("cut_sphere")
    got = _run([(verts, faces)], 0)
    assert torch.equal(got.verts.cpu().view(torch.int32), torch.as_tensor(verts).view(torch.int32))
    _check(got, [_want("cut_sphere", 0)], "iters 0")


def test_a_hub_of_300_spokes_is_ranked_by_a_wave():
    want = _want("cone", 4)
    assert want["degree_max"] == 300 and want["free"] == 302
    _check(_run([_mesh("cone")], 4), [want], "cone")
    _check(_run([_mesh("cone")], 2, 1.0, 0.0), [_want("cone", 2, 1.0, 0.0)], "cone, laplacian")


def test_a_batch_of_three_images_with_an_empty_one_in_the_middle():
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    nothing = dict(verts=np.zeros((0, 3), np.float32), free=0, fixed_boundary=0, isolated=0, degree_max=0, rough_before=0.0, rough_after=0.0,
                   disp_mean=0.0, disp_max=0.0)
    batch = _run([_mesh("cut_sphere"), empty, _mesh("torus")], 2)
    _check(batch, [_want("cut_sphere", 2), nothing, _want("torus", 2)], "batch")
    first, last = _run([_mesh("cut_sphere")], 2), _run([_mesh("torus")], 2)            # each image alone: the same bits
    n = first.verts.shape[0]
    assert torch.equal(batch.verts[:n].view(torch.int32), first.verts.view(torch.int32))
    assert torch.equal(batch.verts[n:].view(torch.int32), last.verts.view(torch.int32))
    for k in ref.INTS + ref.MEASURES:
        view = torch.int64
        assert torch.equal(getattr(batch, k)[[0, 2]].view(view), torch.cat([getattr(first, k), getattr(last, k)]).view(view)), k
    _check(_run([empty], 3), [nothing], "no vertex and no face at all")
    points = np.arange(12, dtype=np.float32).reshape(4, 3)                              # vertices without a face stay where they are
    only = _run([(points, empty[1])], 3)
    assert torch.equal(only.verts.cpu(), torch.as_tensor(points)) and only.isolated.tolist() == [4] and only.free.tolist() == [0]


def test_table_size_face_order_second_run_and_side_stream_change_no_bit():
    verts, faces = _mesh("cut_sphere")
    first = _bits(_run([(verts, faces)], 5))
    _check(_run([(verts, faces)], 5), [_want("cut_sphere", 5)], "second run")
    slots = 1 << (3 * len(faces)).bit_length()                                         # the smallest table: long probe chains
    assert slots > 3 * len(faces)
    perm = np.random.RandomState(5).permutation(len(faces))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        on_side = _bits(_run([(verts, faces)], 5))
    torch.cuda.synchronize()
    for what, other in (("second run", _bits(_run([(verts, faces)], 5))), ("small table", _bits(_run([(verts, faces)], 5, table_slots=slots))),
                        ("large table", _bits(_run([(verts, faces)], 5, table_slots=8 * slots))), ("side stream", on_side)):
        for a, b in zip(first, other):
            assert torch.equal(a, b), what
    permuted = _bits(_run([(verts, np.roll(faces[perm], 1, axis=1))], 5))
    for k, (a, b) in enumerate(zip(first, permuted)):
        assert k == 1 or torch.equal(a, b), ("permuted faces", k)                       # field 1 is the face list itself


def test_a_vertex_that_is_not_finite_raises():
    verts, faces = _mesh("sphere")
    for value in (float("nan"), float("inf"), -float("inf")):
        bad = verts.copy()
        bad[7, 1] = value
        with pytest.raises(ValueError, match="a vertex is not finite"):
            _run([(bad, faces)], 2)
    with pytest.raises(ValueError, match="a vertex is not finite"):                     # a batch: the second image's last vertex
        bad = verts.copy()
        bad[-1, 2] = float("nan")
        _run([(verts, faces), (bad, faces)], 2)
    _check(_run([(verts, faces)], 2), [_want("sphere", 2)], "after a refusal")


def test_a_face_index_out_of_range_raises():
    verts, faces = _mesh("sphere")
    for bad_index in (len(verts), -1, 2 ** 31 - 1):                                     # flagged on the device, never dereferenced
        bad = faces.copy()
        bad[7, 1] = bad_index
        with pytest.raises(ValueError, match="vertex range"):
            _run([(verts, bad)], 2)
    with pytest.raises(ValueError, match="vertex range"):                               # 4 is in the batch's range, not in the second image's
        _run([(verts, faces), (topo.TET_V, np.array([[4, 1, 2]], np.int32))], 2)
    _check(_run([(verts, faces)], 2), [_want("sphere", 2)], "after a refusal")


def test_refusals_before_any_launch_and_of_the_entry_point(monkeypatch):
    from shapeclipper_amd import _lib, ops
    verts, faces = (torch.as_tensor(x).to(DEV) for x in _mesh("sphere"))
    V, F = verts.shape[0], faces.shape[0]
    vc, fc = torch.tensor([V]), torch.tensor([F])
    call = lambda iters=2, lam=0.5, mu=-0.5, slots=None, v=verts, f=faces, nv=vc, nf=fc: ops.mesh_smooth(v, f, nv, nf, iters, lam, mu, slots)
    lib = _lib.load()

    def no_launch():
        raise AssertionError("the library was asked for before the arguments were refused")

    monkeypatch.setattr(_lib, "load", no_launch)
    for kw, name in ((dict(iters=-1), "iters"), (dict(iters=1001), "iters"), (dict(iters=2.0), "iters"), (dict(iters=True), "iters"),
                     (dict(iters=None), "iters"), (dict(lam=0.0), "lam"), (dict(lam=1.5), "lam"), (dict(lam=float("nan")), "lam"),
                     (dict(lam=True), "lam"), (dict(lam="0.5"), "lam"), (dict(mu=0.1), "mu"), (dict(mu=-1.5), "mu"), (dict(mu=float("nan")), "mu"),
                     (dict(mu=-float("inf")), "mu"), (dict(mu=False), "mu"), (dict(slots=3 * F), "table_slots"),
                     (dict(slots=(1 << (3 * F).bit_length()) + 2), "table_slots"), (dict(slots=1 << 31), "table_slots"),
                     (dict(slots=4096.0), "table_slots"), (dict(v=verts.double()), "verts"), (dict(f=faces.long()), "faces"),
                     (dict(v=verts.cpu()), "verts"), (dict(f=faces.cpu()), "faces"), (dict(v=verts[:, :2]), "verts"),
                     (dict(nv=torch.tensor([5])), "v_count"), (dict(nf=torch.tensor([F, -1])), "v_count"), (dict(nv=vc.float()), "v_count")):
        with pytest.raises(ValueError, match=name):
            call(**kw)
    monkeypatch.undo()
    T = ops.mesh_topology_slots(F)
    assert lib.sc_mesh_smooth_scratch_bytes(1, V, F, T) > 0 and lib.sc_mesh_smooth_scratch_bytes(3, 0, 0, 2) > 0
    for sizes in ((1, V, F, 0), (1, V, F, T + 2), (1, V, F, 512), (0, V, F, T), (65536, V, F, T), (1, V, (1 << 26) + 1, 1 << 30), (1, -1, F, T),
                  (1, (1 << 30) + 1, F, T)):
        assert lib.sc_mesh_smooth_scratch_bytes(*sizes) == 0, sizes
    off = torch.tensor([[0, V], [0, F]], dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.sc_mesh_smooth_scratch_bytes(1, V, F, T) // 4 + 8, device=DEV)
    out_v = torch.empty(V, 3, device=DEV)
    counts, measures = torch.empty(4, 1, dtype=torch.int64, device=DEV), torch.empty(4, 1, dtype=torch.float64, device=DEV)
    bad = torch.empty(2, dtype=torch.int32, device=DEV)
    p = _lib.ptr

    def entry(verts_=verts, slots=T, iters=2, lam=0.5, mu=ref.MU, scratch=ws.data_ptr(), counts_=counts, n_faces=F, out=out_v):
        return lib.sc_mesh_smooth(p(verts_), p(faces), p(off[0]), p(off[1]), 1, V, n_faces, slots, iters, lam, mu, scratch, p(out), p(counts_),
                                  p(measures), p(bad[:1]), p(bad[1:]), _lib.stream())
    INVALID = 1                                                                         # hipErrorInvalidValue
    for kw in (dict(verts_=None), dict(out=None), dict(counts_=None), dict(scratch=None), dict(scratch=ws.data_ptr() + 4), dict(slots=512),
               dict(slots=T + 2), dict(iters=-1), dict(iters=1001), dict(lam=0.0), dict(lam=float("nan")), dict(lam=1.25), dict(mu=0.5),
               dict(mu=float("nan")), dict(mu=-1.5), dict(n_faces=(1 << 26) + 1)):
        assert entry(**kw) == INVALID, kw
    assert entry() == 0
    torch.cuda.synchronize()
    want = _want("sphere", 2)
    assert bad.tolist() == [0, 0] and counts[:, 0].tolist() == [want[k] for k in ref.INTS]
    assert torch.equal(out_v.cpu().view(torch.int32), torch.as_tensor(want["verts"]).view(torch.int32))
    _check(call(mu=ref.MU), [want], "after the refusals")
