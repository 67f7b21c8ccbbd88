"""Dual contouring on the GPU (ops.dual_contour_mesh, csrc/dual_contour.hip) and the evaluation's `--eval.dual_mesh` dump.

The rule: vertices, faces and counts are bit-identical to the numpy restatement of the header's text (tests/dual_contour_ref.py).  On top
of that the properties the feature is for: a box keeps its corners where marching cubes chamfers them, closed surfaces give closed,
consistently oriented manifolds, every vertex stays in its cell, and the switch adds {idx}_mesh_dual.ply without moving another byte."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dual_contour_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _grids():
    return R.grids()


@functools.lru_cache(maxsize=None)
def _ref(name, iso=0.0, reg=0.05):
    level, normals = _grids()[name]
    return R.dual_contour(level, normals, iso, reg)


def _run(names, iso=0.0, reg=0.05):
    from shapeclipper_amd import ops
    level = torch.tensor(np.stack([_grids()[n][0] for n in names])).cuda()
    normals = torch.tensor(np.concatenate([_grids()[n][1] for n in names]).reshape(-1, 3)).cuda()
    return ops.dual_contour_mesh(level, normals, iso, reg)


def _split(verts, faces, vc, fc):
    v_end, f_end = np.cumsum(vc.numpy()).tolist(), np.cumsum(fc.numpy()).tolist()
    return [(verts[v_end[b] - int(vc[b]):v_end[b]].cpu().numpy(), faces[f_end[b] - int(fc[b]):f_end[b]].cpu().numpy()) for b in range(len(vc))]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


def _check_against_ref(names):
    verts, faces, vc, fc = out = _run(names)
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32 and verts.is_cuda and faces.is_cuda
    assert vc.dtype == fc.dtype == torch.int64 and not vc.is_cuda and not fc.is_cuda
    assert verts.shape == (int(vc.sum()), 3) and faces.shape == (int(fc.sum()), 3)
    for name, (v, f) in zip(names, _split(*out)):
        want_v, want_f = _ref(name)
        assert v.shape[0] == want_v.shape[0] and f.shape[0] == want_f.shape[0], name
        assert np.array_equal(f, want_f), name
        assert _same_bits(v, want_v), (name, np.abs(v - want_v).max())
    return out


@pytest.mark.parametrize("names", [("sphere",), ("torus",), ("noise0", "noise1", "noise2"), ("nans",), ("s2",), ("s3",), ("box",),
                                   ("noise0", "outside", "noise2")], ids="+".join)
def test_bit_for_bit_against_the_fp32_restatement(names):
    _, _, vc, fc = _check_against_ref(names)
    if "outside" in names:                                      # an image with no surface yields nothing, between two that have one
        assert vc[1] == fc[1] == 0 and vc[0] > 0 and vc[2] > 0
    if names == ("nans",):
        level, normals = _grids()["nans"]
        assert np.isnan(level).sum() == 1 and np.isnan(R.crossings(level)[0]).any(1).sum() >= 1 and np.isnan(normals).any(1).sum() >= 2
        assert np.isfinite(_ref("nans")[0]).all()               # the clamp leaves no NaN behind


def test_no_surface_at_all():
    verts, faces, vc, fc = _run(("outside", "outside"))
    assert verts.shape == (0, 3) and faces.shape == (0, 3) and vc.tolist() == fc.tolist() == [0, 0]


def test_sharpness():
    """The point of the feature.  The exact SDF of the box [2.5, 8.5]^3 on S = 12 with the axis normals of the crossed faces: in a corner
    cell the three tangent planes meet at the corner, 1/3 per axis from the mean of the crossings, and the regularisation keeps
    1 / (1 + 3 reg) of that offset: the vertex ends sqrt(3) (1/3) (0.15 / 1.15) = 0.075 from the corner, within 0.1.  Marching cubes has
    no vertex within 0.7: its nearest sits on a grid edge sqrt(0.5) away.  Every dual vertex lies within 0.1 of the box surface."""
    from shapeclipper_amd import ops
    level, normals = _grids()["box"]
    (v, f), = _split(*_run(("box",)))
    corners = np.array([[a, b, c] for a in (2.5, 8.5) for b in (2.5, 8.5) for c in (2.5, 8.5)])
    dist = np.linalg.norm(v[None].astype(np.float64) - corners[:, None], axis=2).min(1)
    print("nearest dual vertex to each corner:", dist)
    assert (dist <= 0.1).all()
    mc = ops.isosurface_mesh(torch.tensor(level[None]).cuda())[0].cpu().numpy()
    mc_dist = np.linalg.norm(mc[None].astype(np.float64) - corners[:, None], axis=2).min(1)
    print("nearest marching-cubes vertex to each corner:", mc_dist)
    assert (mc_dist >= 0.7).all()
    q = np.abs(v.astype(np.float64) - 5.5) - 3.0                # the box SDF at every dual vertex
    sdf = np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(1), 0)
    print("largest |box sdf| at a dual vertex:", np.abs(sdf).max())
    assert (np.abs(sdf) <= 0.1).all()


def _signed_volume(v, f):
    t = v.astype(np.float64)[f]
    return float(np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6)


def _interior_crossing_edges(level, iso=0.0):
    S, inside, n = level.shape[0], level < np.float32(iso), 0
    for a in range(3):
        lo, hi = [slice(1, S - 1)] * 3, [slice(1, S - 1)] * 3
        lo[a], hi[a] = slice(0, S - 1), slice(1, S)
        n += int((inside[tuple(lo)] != inside[tuple(hi)]).sum())
    return n


def _owning_cells(level, iso=0.0):
    S, inside = level.shape[0], level < np.float32(iso)
    n = sum(inside[dx:S - 1 + dx, dy:S - 1 + dy, dz:S - 1 + dz].astype(np.int32) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1))
    return np.argwhere((n > 0) & (n < 8))                       # ascending linear cell index


@pytest.mark.parametrize("name,chi", [("sphere", 2), ("torus", 0)])
def test_it_is_a_mesh(name, chi):
    from shapeclipper_amd import ops
    level = _grids()[name][0]
    verts, faces, vc, fc = _run((name,))
    (v, f), = _split(verts, faces, vc, fc)
    V, F = v.shape[0], f.shape[0]
    assert f.min() >= 0 and f.max() < V and np.bincount(f.reshape(-1), minlength=V).min() >= 1
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64)
    key, rev = directed[:, 0] * V + directed[:, 1], directed[:, 1] * V + directed[:, 0]
    assert np.unique(key).shape[0] == 3 * F                     # every directed edge once ...
    assert np.array_equal(np.sort(key), np.sort(rev))           # ... and matched by its opposite
    E = np.unique(np.sort(directed, 1), axis=0).shape[0]
    assert V - E + F == chi
    mv, mf, _, _ = ops.isosurface_mesh(torch.tensor(level[None]).cuda())
    vol, mc_vol = _signed_volume(v, f), _signed_volume(mv.cpu().numpy(), mf.cpu().numpy())
    print(name, "signed volume: dual", vol, "marching cubes", mc_vol)
    assert vol * mc_vol > 0
    assert int(fc[0]) == 2 * _interior_crossing_edges(level)


@pytest.mark.parametrize("name", ["sphere", "torus", "noise1", "nans", "box", "s2", "s3"])
def test_every_vertex_lies_in_its_own_cell(name):
    level = _grids()[name][0]
    (v, _), = _split(*_run((name,)))
    cells = _owning_cells(level).astype(np.float32)
    assert cells.shape == v.shape
    assert ((v >= cells) & (v <= cells + 1)).all()


def test_determinism_batching_and_iso():
    from shapeclipper_amd import ops
    names = ("noise0", "sphere9", "outside", "noise2")
    grids = dict(_grids())
    grids["sphere9"] = R.sphere(9, 0.6, (0.0, 0.1, -0.1))
    level = torch.tensor(np.stack([grids[n][0] for n in names])).cuda()
    normals = torch.tensor(np.concatenate([grids[n][1] for n in names])).cuda()
    a, b = ops.dual_contour_mesh(level, normals), ops.dual_contour_mesh(level, normals)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    for i, (v, f) in enumerate(_split(*a)):
        nr = torch.tensor(grids[names[i]][1]).cuda()
        vs, fs, vc, fc = ops.dual_contour_mesh(level[i:i + 1], nr)
        assert int(vc[0]) == v.shape[0] and int(fc[0]) == f.shape[0]
        assert _same_bits(vs.cpu().numpy(), v) and np.array_equal(fs.cpu().numpy(), f)
    # a non-zero iso agrees with the shifted grid: values on a 1/64 lattice, so level - iso and every difference are exact in fp32
    iso = 0.25
    q = (np.round(grids["noise1"][0] * 64) / 64).astype(np.float32)
    nq = R.finite_difference_normals(q, iso)
    want_v, want_f = R.dual_contour(q, nq, iso, 0.05)
    got = ops.dual_contour_mesh(torch.tensor(q[None]).cuda(), torch.tensor(nq).cuda(), iso)
    shifted = ops.dual_contour_mesh(torch.tensor((q - np.float32(iso))[None]).cuda(), torch.tensor(nq).cuda(), 0.0)
    assert want_v.shape[0] > 0 and want_f.shape[0] > 0
    assert _same_bits(got[0].cpu().numpy(), want_v) and np.array_equal(got[1].cpu().numpy(), want_f)
    assert all(torch.equal(x, y) for x, y in zip(got, shifted))


def test_refusals():
    from shapeclipper_amd import ops
    level, normals = _grids()["noise0"]
    lv, nr = torch.tensor(level[None]).cuda(), torch.tensor(normals).cuda()
    for bad in (nr[:-1], torch.cat([nr, nr[:1]]), nr[:0]):
        with pytest.raises(ValueError, match="normals"):
            ops.dual_contour_mesh(lv, bad)
    with pytest.raises(ValueError, match="normals"):
        ops.dual_contour_mesh(lv, nr.cpu())
    with pytest.raises(ValueError, match="reg"):
        ops.dual_contour_mesh(lv, nr, 0.0, 0.0)
    with pytest.raises(RuntimeError, match="grid side"):        # isosurface_mesh's refusal
        ops.dual_contour_mesh(torch.zeros(1, 1, 1, 1, device="cuda"), torch.zeros(0, 3, device="cuda"))


# ---- end to end: the evaluation's dumps --------------------------------------------------------------------------------------------
def _read_ply(fname):
    data = open(fname, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[1] == "format binary_little_endian 1.0"
    props = [l.split()[2] for l in lines if l.startswith("property float")]
    n_v = int([l for l in lines if l.startswith("element vertex")][0].split()[2])
    n_f = int([l for l in lines if l.startswith("element face")][0].split()[2])
    vdt = np.dtype([(p, "<f4") for p in props])
    v = np.frombuffer(data, vdt, n_v, end)
    rec = np.frombuffer(data, np.dtype([("n", "u1"), ("i", "<i4", (3,))]), n_f, end + vdt.itemsize * n_v)
    assert (rec["n"] == 3).all() and end + vdt.itemsize * n_v + 13 * n_f == len(data)
    return props, np.stack([v["x"], v["y"], v["z"]], 1), rec["i"]


def test_evaluate_writes_dual_meshes(tmp_path):
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    from shapeclipper_amd.model.runner import Runner
    from shapeclipper_amd.utils import eval_3D, options
    from shapeclipper_amd.utils.util import EasyDict as edict
    o = options.set(options.parse_arguments(["--yaml=options/pix3d/config.yaml", "--name=pytest_dual_mesh", "--output_root=%s" % tmp_path,
                                             "--arch.enc_pretrained!", "--data.dataset=synthetic", "--eval.vox_res=16",
                                             "--eval.num_points=1000", "--tb!", "--eval.dual_mesh"]), verbose=False)
    o.device, o.world_size, o.port = 0, 1, 0
    torch.manual_seed(0)
    r = Runner(o)
    r.load_dataset(o, eval_split="test")
    r.build_networks(o)
    net = r.graph.module
    seen = []
    dump = r.dump_visuals

    def spy(opt, var, ep, train=False):
        seen.append((var.idx.cpu().tolist(), var.level_vox.clone(), var.proj_latent_sdf.clone()))
        return dump(opt, var, ep, train=train)

    out = os.path.join(o.output_path, "dump")
    files = lambda: {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out)) if f.endswith(".ply")}
    texts = lambda: tuple(open(os.path.join(o.output_path, f)).read() for f in ("chamfer.txt", "f_score.txt"))
    lo, hi = o.eval.range
    pitch = (hi - lo) / o.eval.vox_res
    r.dump_visuals = spy
    results = {}
    for mode in ("evaluate", "evaluate_sharded"):
        seen.clear()
        for f in os.listdir(out) if os.path.isdir(out) else []:
            os.remove(os.path.join(out, f))
        o.eval.dual_mesh = True
        getattr(r, mode)(o, ep=0)
        on_files, on_texts = files(), texts()
        n_dual = 0
        for ids, level, zs in seen:
            meshes = eval_3D.meshes_dual(o, net.sdf_network, zs, level, 0.05)
            for (v_, f_), i in zip(meshes, ids):
                name = "%d_mesh_dual.ply" % i
                if f_.shape[0] == 0:
                    assert name not in on_files
                    continue
                props, v, f = _read_ply(os.path.join(out, name))
                assert props == ["x", "y", "z"]                              # positions and faces, nothing else
                assert np.array_equal(v, v_.cpu().numpy()) and np.array_equal(f, f_.cpu().numpy())
                assert f.min() >= 0 and f.max() < v.shape[0]
                _, mv, _ = _read_ply(os.path.join(out, "%d_mesh.ply" % i))
                assert (v.min(0) >= mv.min(0) - pitch).all() and (v.max(0) <= mv.max(0) + pitch).all()
                n_dual += 1
        assert n_dual >= 1, mode
        # the switch off: no dual file, every other file and the metrics byte-identical
        for f in os.listdir(out):
            os.remove(os.path.join(out, f))
        del o.eval.dual_mesh                                    # absent means off
        getattr(r, mode)(o, ep=0)
        off_files = files()
        assert not any("dual" in f for f in off_files)
        assert off_files == {k: v for k, v in on_files.items() if not k.endswith("_mesh_dual.ply")}
        assert any(k.endswith("_mesh.ply") for k in off_files) and texts() == on_texts
        results[mode] = on_files
    assert results["evaluate"].keys() == results["evaluate_sharded"].keys()
    # vis_{ep}/ of the training-time visualisation goes through the same dump_geometry
    r.dump_visuals = dump
    r.graph.eval()
    o.eval.dual_mesh = True
    o.H, o.W = o.eval.image_size
    os.makedirs(os.path.join(o.output_path, "vis_3"), exist_ok=True)
    n_dual = 0
    for it in range(len(r.test_data)):
        sample = r.test_data[it]
        batch = {k: ({kk: vv[None] for kk, vv in v.items()} if isinstance(v, dict) else torch.as_tensor(v)[None]) for k, v in sample.items()}
        with torch.no_grad():
            var = r.evaluate_batch(o, edict(batch), 0, 0, single_gpu=True)
            eval_3D.eval_metrics(o, var, net.sdf_network, vis_only=True)
            r.dump_geometry(o, var, "vis_3")
        names = os.listdir(os.path.join(o.output_path, "vis_3"))
        i = int(var.idx[0])
        assert ("%d_mesh.ply" % i in names) == ("%d_mesh_dual.ply" % i in names)
        n_dual += "%d_mesh_dual.ply" % i in names
    assert n_dual >= 1
