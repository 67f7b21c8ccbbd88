"""Indexed marching-cubes mesh on the GPU (ops.isosurface_mesh, csrc/isosurface.hip) and the evaluation's PLY dumps.

What is pinned: the faces ARE the soup of ops.isosurface_triangles (verts[faces] equal bit for bit, same order); the vertices are the
sign-changing grid edges in (owner point, axis) order at the soup's interpolation (numpy restatement below); the result is a mesh
(every vertex used, closed and consistently oriented on closed surfaces, Euler characteristic of a sphere and a torus); Runner.evaluate /
evaluate_sharded write {idx}_mesh.ply and {idx}_pointclouds_comp.ply without moving the metrics."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _sphere(S, r, centre=(0.0, 0.0, 0.0)):
    ax = np.linspace(-1, 1, S)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    return (np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) - r).astype(np.float32)


def _torus(S, R, r):
    ax = np.linspace(-1, 1, S)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    return (np.sqrt((np.sqrt(X * X + Y * Y) - R) ** 2 + Z * Z) - r).astype(np.float32)


def _noise_closed(S, seed):
    g = np.random.RandomState(seed).randn(S, S, S).astype(np.float32)
    g[[0, -1]] = 1.0; g[:, [0, -1]] = 1.0; g[:, :, [0, -1]] = 1.0          # outside on the boundary shell: the surface closes
    return g


def crossing_vertices_in_order(level, iso=0.0):
    """Numpy restatement of the vertex contract: one vertex per grid edge (p, p + e_axis) whose ends lie on different sides of iso
    (inside = value < iso), ordered by the linear index of p, then axis; the interpolation of oracle/isosurface_ref.crossing_edge_vertices."""
    level = np.asarray(level, dtype=np.float32)
    S = level.shape[0]
    idx = np.stack(np.meshgrid(np.arange(S), np.arange(S), np.arange(S), indexing="ij"), -1)
    keys, pts = [], []
    for axis in range(3):
        lo = [slice(None)] * 3; hi = [slice(None)] * 3
        lo[axis] = slice(0, S - 1); hi[axis] = slice(1, S)
        fa, fb = level[tuple(lo)], level[tuple(hi)]
        cross = (fa < iso) != (fb < iso)
        t = (np.float32(iso) - fa[cross]) / (fb[cross] - fa[cross])
        owner = idx[tuple(lo)][cross]
        p = owner.astype(np.float32)
        p[:, axis] = p[:, axis] + t * np.float32(1.0)
        keys.append(((owner[:, 0].astype(np.int64) * S + owner[:, 1]) * S + owner[:, 2]) * 3 + axis)
        pts.append(p)
    keys, pts = np.concatenate(keys), np.concatenate(pts).astype(np.float32)
    return pts[np.argsort(keys, kind="stable")]


def _split(verts, faces, vc, fc):
    v_end, f_end = np.cumsum(vc.numpy()).tolist(), np.cumsum(fc.numpy()).tolist()
    return [(verts[v_end[b] - int(vc[b]):v_end[b]], faces[f_end[b] - int(fc[b]):f_end[b]]) for b in range(len(vc))]


def _check_faces_are_soup(level, iso=0.0):
    from shapeclipper_amd import ops
    lv = torch.tensor(level).cuda() if isinstance(level, np.ndarray) else level
    verts, faces, vc, fc = ops.isosurface_mesh(lv, iso)
    tris, per = ops.isosurface_triangles(lv, iso)
    assert vc.dtype == fc.dtype == torch.int64 and not vc.is_cuda and not fc.is_cuda
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32 and verts.is_cuda and faces.is_cuda
    assert fc.tolist() == per.tolist() and faces.shape == (int(fc.sum()), 3) and verts.shape == (int(vc.sum()), 3)
    soup = torch.cat([v[f.long()] for v, f in _split(verts, faces, vc, fc)]) if faces.shape[0] else torch.zeros(0, 3, 3, device="cuda")
    assert torch.equal(soup, tris)
    return verts, faces, vc, fc


def test_faces_are_the_soup_bit_for_bit():
    rng = np.random.RandomState(0)
    tie = _sphere(13, 0.5)
    tie[6, 6, 1] = 0.0                                                       # an exact 0.0 on a grid point
    empty = np.full((7, 7, 7), 1.0, np.float32)
    for g in [rng.randn(7, 7, 7).astype(np.float32) for _ in range(3)] + [_sphere(13, 0.55, (0.1, -0.05, 0.2)), tie, empty]:
        _check_faces_are_soup(g[None])
    _, _, vc, fc = _check_faces_are_soup(empty[None])
    assert vc.tolist() == fc.tolist() == [0]
    a, c = _sphere(9, 0.5), _sphere(9, 0.7, (0.1, 0.1, 0.0))
    _, _, vc, fc = _check_faces_are_soup(np.stack([a, np.full((9, 9, 9), -1.0, np.float32), c]))
    assert vc[1] == fc[1] == 0 and vc[0] > 0 and vc[2] > 0
    for g in (np.array([[[-1, 1], [1, 1]], [[1, 1], [1, 0.5]]], np.float32), rng.randn(2, 2, 2).astype(np.float32)):   # S = 2
        _check_faces_are_soup(g[None])
    big = np.stack([_sphere(101, r, (0.05 * k, 0.0, -0.03 * k)) for k, r in enumerate((0.3, 0.5, 0.7, 0.9))])
    _check_faces_are_soup(big)


def test_vertex_set_and_order():
    from oracle.isosurface_ref import crossing_edge_vertices
    from shapeclipper_amd import ops
    rng = np.random.RandomState(1)
    tie = _sphere(13, 0.5)
    tie[6, 6, 1] = 0.0
    for g, iso in ((rng.randn(7, 7, 7).astype(np.float32), 0.0), (_sphere(13, 0.55, (0.1, -0.05, 0.2)), 0.0), (tie, 0.0),
                   (_torus(33, 0.5, 0.2), 0.03), (rng.randn(19, 19, 19).astype(np.float32), -0.2)):
        verts, faces, vc, fc = ops.isosurface_mesh(torch.tensor(g[None]).cuda(), iso)
        want = crossing_vertices_in_order(g, iso)
        got = verts.cpu().numpy()
        assert int(vc[0]) == want.shape[0] and np.array_equal(got, want)
        assert np.array_equal(got[np.lexsort((got[:, 2], got[:, 1], got[:, 0]))], crossing_edge_vertices(g, iso))


def _check_mesh(verts, faces, closed, manifold=True):
    """closed: every directed edge is matched by its reverse (no boundary, one consistent orientation); manifold: moreover every
    directed edge occurs once and every undirected edge lies in exactly two faces.  Returns V - E + F of a closed mesh."""
    V, F = verts.shape[0], faces.shape[0]
    f = faces.long().cpu().numpy()
    assert f.min() >= 0 and f.max() < V
    assert np.bincount(f.reshape(-1), minlength=V).min() >= 1                        # every vertex is used
    assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])).all()  # three distinct corners
    if not closed:
        return None
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = directed[:, 0] * V + directed[:, 1]
    rev = directed[:, 1] * V + directed[:, 0]
    assert np.array_equal(np.sort(key), np.sort(rev))                                # each directed edge meets its reverse as often
    undirected, uses = np.unique(np.sort(directed, 1), axis=0, return_counts=True)
    if manifold:
        assert np.unique(key).shape[0] == 3 * F                                      # every directed edge once
        assert (uses == 2).all()                                                     # every edge in exactly two faces
    return V - undirected.shape[0] + F


def test_it_is_a_mesh():
    _check_faces_are_soup(_sphere(33, 0.5)[None])
    from shapeclipper_amd import ops
    for g, chi in ((_sphere(33, 0.5), 2), (_torus(33, 0.5, 0.2), 0)):
        verts, faces, vc, fc = ops.isosurface_mesh(torch.tensor(g[None]).cuda())
        assert _check_mesh(verts, faces, closed=True) == chi
    # noise: closed and consistently oriented.  Not always a 2-manifold: where an ambiguous face of two neighbouring cubes has both cubes'
    # fan triangulations draw the same chord across it, that edge lies in four faces (twice per direction) -- a property of the soup's
    # table (csrc/mc_table.hpp), which the faces reproduce exactly; seeds 2 and 3 each hold two such edges.
    for seed in (2, 3):
        g = _noise_closed(15, seed)
        verts, faces, _, _ = _check_faces_are_soup(g[None])
        _check_mesh(verts, faces, closed=True, manifold=False)
    rng = np.random.RandomState(4)
    verts, faces, _, _ = _check_faces_are_soup(rng.randn(1, 11, 11, 11).astype(np.float32))
    _check_mesh(verts, faces, closed=False)


def test_determinism_batching_and_iso():
    from shapeclipper_amd import ops
    rng = np.random.RandomState(5)
    S = 37                                                                   # 37^3 points: no multiple of the 1,024-point block
    batch = np.stack([_sphere(S, 0.5, (0.1, 0.0, -0.2)), rng.randn(S, S, S).astype(np.float32), np.full((S, S, S), 2.0, np.float32),
                      _torus(S, 0.5, 0.25)])
    lv = torch.tensor(batch).cuda()
    a, b = ops.isosurface_mesh(lv), ops.isosurface_mesh(lv)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    for i, (v, f) in enumerate(_split(*a)):
        vs, fs, vc, fc = ops.isosurface_mesh(lv[i:i + 1])
        assert int(vc[0]) == v.shape[0] and int(fc[0]) == f.shape[0] and torch.equal(vs, v) and torch.equal(fs, f)
    for iso in (0.03, -0.4):
        verts, faces, vc, fc = _check_faces_are_soup(lv, iso)
        for i, (v, f) in enumerate(_split(verts, faces, vc, fc)):
            assert np.array_equal(v.cpu().numpy(), crossing_vertices_in_order(batch[i], iso))


def test_bad_grid_side_raises():
    from shapeclipper_amd import ops
    with pytest.raises(RuntimeError, match="grid side"):
        ops.isosurface_mesh(torch.zeros(1, 1, 1, 1, device="cuda"))


# ---- end to end: the evaluation's dumps --------------------------------------------------------------------------------------------
def read_ply(fname):
    data = open(fname, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[1] == "format binary_little_endian 1.0"
    n_v = int([l for l in lines if l.startswith("element vertex")][0].split()[2])
    n_f = [int(l.split()[2]) for l in lines if l.startswith("element face")]
    colours = "property uchar red" in lines
    vdt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if colours else []))
    verts = np.frombuffer(data, vdt, n_v, end)
    faces = None
    if n_f:
        fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
        rec = np.frombuffer(data, fdt, n_f[0], end + vdt.itemsize * n_v)
        assert (rec["n"] == 3).all()
        faces = rec["i"]
    assert end + vdt.itemsize * n_v + (13 * n_f[0] if n_f else 0) == len(data)
    return verts, faces


def _xyz(v):
    return np.stack([v["x"], v["y"], v["z"]], 1)


def test_evaluate_writes_meshes_and_pointclouds(tmp_path):
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    from shapeclipper_amd import ops
    from shapeclipper_amd.model.runner import Runner
    from shapeclipper_amd.utils import options
    o = options.set(options.parse_arguments(["--yaml=options/pix3d/config.yaml", "--name=pytest_mesh", "--output_root=%s" % tmp_path,
                                             "--arch.enc_pretrained!", "--data.dataset=synthetic", "--eval.vox_res=16",
                                             "--eval.num_points=1000", "--tb!"]), verbose=False)
    o.device, o.world_size, o.port = 0, 1, 0
    torch.manual_seed(0)
    r = Runner(o)
    r.load_dataset(o, eval_split="test")
    r.build_networks(o)
    seen = []
    dump = r.dump_visuals

    def spy(opt, var, ep, train=False):
        seen.append((var.idx.cpu().tolist(), var.level_vox.clone(), var.dpc_pred.clone(), var.dpc.points.clone()))
        return dump(opt, var, ep, train=train)

    r.dump_visuals = spy
    r.evaluate(o, ep=0)
    out = os.path.join(o.output_path, "dump")
    chamfer, fscore = open(os.path.join(o.output_path, "chamfer.txt")).read(), open(os.path.join(o.output_path, "f_score.txt")).read()
    idxs = sorted(i for s in seen for i in s[0])
    assert idxs == list(range(len(r.test_data))) and len(idxs) == 4
    lo, hi = o.eval.range
    first = {}
    n_meshes = 0
    for ids, level, dpc_pred, dpc_gt in seen:
        S = level.shape[1]
        _, _, vc, fc = ops.isosurface_mesh(level)
        tris, per = ops.isosurface_triangles(level)
        soup = (tris / S * (hi - lo) + lo).cpu().numpy()
        ends = np.cumsum(per.numpy()).tolist()
        for b, i in enumerate(ids):
            mesh_file = os.path.join(out, "%d_mesh.ply" % i)
            if int(fc[b]) == 0:
                assert not os.path.exists(mesh_file)
            else:
                v, f = read_ply(mesh_file)
                assert v.shape[0] == int(vc[b]) and f.shape[0] == int(fc[b])
                assert np.array_equal(_xyz(v)[f], soup[ends[b] - int(per[b]):ends[b]])
                first[i] = (_xyz(v), f)
                n_meshes += 1
            c, _ = read_ply(os.path.join(out, "%d_pointclouds_comp.ply" % i))
            assert c.shape[0] == 2 * 1000
            assert np.array_equal(_xyz(c), np.concatenate([dpc_pred[b].cpu().numpy(), dpc_gt[b].cpu().numpy()]))
            rgb = np.stack([c["red"], c["green"], c["blue"]], 1)
            assert (rgb[:1000] == [255, 0, 0]).all() and (rgb[1000:] == [0, 255, 0]).all()
    assert n_meshes >= 1
    for f in os.listdir(out):
        if f.endswith(".ply"):
            os.remove(os.path.join(out, f))
    # the sharded evaluation (world 1) writes the same files for its samples
    r.dump_visuals = dump
    r.evaluate_sharded(o, ep=0)
    for i, (v0, f0) in first.items():
        v, f = read_ply(os.path.join(out, "%d_mesh.ply" % i))
        assert v.shape[0] == v0.shape[0] and f.shape[0] == f0.shape[0]
        assert np.abs(_xyz(v) - v0).max() <= 1e-6
    for i in idxs:
        c, _ = read_ply(os.path.join(out, "%d_pointclouds_comp.ply" % i))
        assert c.shape[0] == 2000
    # the metrics do not depend on the dumps
    r.dump_visuals = lambda *a, **k: None
    r.evaluate(o, ep=0)
    assert open(os.path.join(o.output_path, "chamfer.txt")).read() == chamfer
    assert open(os.path.join(o.output_path, "f_score.txt")).read() == fscore
    r.evaluate_sharded(o, ep=0)
    r.dump_visuals = dump
    sharded_without = open(os.path.join(o.output_path, "chamfer.txt")).read(), open(os.path.join(o.output_path, "f_score.txt")).read()
    r.evaluate_sharded(o, ep=0)
    assert (open(os.path.join(o.output_path, "chamfer.txt")).read(), open(os.path.join(o.output_path, "f_score.txt")).read()) == sharded_without
