"""ops.point_mesh_distance (csrc/point_mesh.hip) on the GPU against the numpy restatement tests/point_mesh_ref.py, bit for bit, the grid
search against the all-pairs twin, and the evaluation's `--eval.mesh_dist` on the pix3d_mini tree (the two-rank run of evaluate.py is in
tests/test_zz_point_mesh_two_ranks.py: tests that start other processes run behind the kernel tests).

Shapes: a few hundred triangles and at most 2,000 queries per case -- every path of the search is taken at that size: cells of the ring
walk, the clamped start outside the box, the large list, the list of queries the walk gives up on (queries several box sizes away lie
more than two cells outside the box: the documented rule sends them to the all-pairs loop), images with an unusable grid."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import point_mesh_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEV = torch.device("cuda:0")


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def _same(got, want, what):
    """got (a tensor) and want (numpy) hold the same bits; NaN matches NaN."""
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind == "f":
        same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    else:
        same = got == want
    assert same.all(), "%s: %d of %d differ, first at %s: got %r, want %r" % (
        what, (~same).sum(), same.size, np.argwhere(~same)[0], got[tuple(np.argwhere(~same)[0])], want[tuple(np.argwhere(~same)[0])])


def _run(case, search):
    from shapeclipper_amd import ops
    pts, verts, faces, v_count, f_count = case
    return ops.point_mesh_distance(_dev(pts), _dev(verts), _dev(faces), _dev(v_count), _dev(f_count), search=search)


def _check(case, want, what):
    for search in ("grid", "brute"):
        got = _run(case, search)
        assert got.dist2.dtype == torch.float32 and got.face.dtype == torch.int32 and got.closest.dtype == torch.float32
        for name, g, w in zip(("dist2", "face", "closest"), got, want):
            _same(g, w, "%s %s %s" % (what, search, name))


@pytest.fixture(scope="module")
def cases():
    cs = ref.cases()
    return {k: (c, ref.point_mesh(*c)) for k, c in cs.items()}


# ---- 1. bits against the restatement, grid == brute ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere", "batch3", "huge", "degenerate", "flat", "n1", "n65", "f1"])
def test_bits_against_the_restatement(cases, name):
    case, want = cases[name]
    _check(case, want, name)
    d, f, q = want
    if name == "sphere":            # queries on vertices and edge midpoints tie between the faces around them: the lowest index is the answer
        assert (d == 0).sum() >= 400 and np.isfinite(d).all() and (f >= 0).all()
        assert d.max() > 4.0        # the far queries
    if name == "batch3":
        assert np.isinf(d[1]).all() and (f[1] == -1).all() and not q[1].any()           # the empty image
        assert np.isfinite(d[0]).all() and np.isfinite(d[2]).all() and f[2].max() <= 200
    if name == "huge":
        assert (f == 0).sum() > 50                                                      # the triangle across the box wins often
    if name == "degenerate":
        assert not np.isnan(d).any() and not np.isnan(q).any()
        assert ((f >= 0) & (f < 50)).sum() > 0 and (f[(f >= 0) & (f < 50)] == 0).all()  # 50 exact duplicates: the lowest index wins
        assert f[0, -24] == 0 and d[0, -24] == 0                                        # a query on a vertex of the duplicated triangle


# ---- 2. non-finite inputs -------------------------------------------------------------------------------------------------------------------
def test_a_nan_query_and_a_nan_vertex_leave_every_other_row_exact(cases):
    (pts, verts, faces, v_count, f_count), _ = cases["n65"]
    pts = np.concatenate([pts, pts], axis=0).copy()
    verts2 = verts.copy()
    pts[0, 7, 1] = np.nan
    pts[1, 9, 0] = np.inf
    verts2[faces[11, 2], 0] = np.nan                    # image 1's mesh: a NaN vertex -- its faces count through their finite edges only, the grid is off
    case = (pts, np.concatenate([verts, verts2]), np.concatenate([faces, faces]), np.tile(v_count, 2), np.tile(f_count, 2))
    want = ref.point_mesh(*case)
    d, f, q = want
    assert np.isnan(d[0, 7]) and f[0, 7] == -1 and np.isnan(q[0, 7]).all() and np.isnan(d[1, 9]) and f[1, 9] == -1
    assert np.isfinite(np.delete(d[0], 7)).all() and np.isfinite(np.delete(d[1], 9)).all()
    _check(case, want, "non-finite")


# ---- 3. the same bits ------------------------------------------------------------------------------------------------------------------------
def test_same_bits_run_to_run_on_a_side_stream_and_in_any_batch(cases):
    from shapeclipper_amd import ops
    case, want = cases["batch3"]
    args = [_dev(x) for x in case]
    first = ops.point_mesh_distance(*args)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = ops.point_mesh_distance(*args)
    again = ops.point_mesh_distance(*args)
    torch.cuda.synchronize()
    for a, b, c in zip(first, other, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))
    pts, verts, faces, v_count, f_count = case
    v0 = f0 = 0
    for b in range(3):
        v1, f1 = v0 + int(v_count[b]), f0 + int(f_count[b])
        one = (pts[b:b + 1], verts[v0:v1], faces[f0:f1], v_count[b:b + 1], f_count[b:b + 1])
        _check(one, tuple(w[b:b + 1] for w in want), "image %d alone" % b)
        v0, f0 = v1, f1


# ---- 4. samples of the surface lie on the mesh ---------------------------------------------------------------------------------------------
def test_surface_samples_lie_on_the_indexed_mesh():
    """surface_points_device samples the triangles meshes_device indexes, so every sample is on the mesh up to rounding.  The yardstick
    is the float64 distance (point_mesh_ref.brute_exact, on the CPU) of those same fp32 samples to the mesh: its largest value times 4
    bounds every fp32 distance.  Measured on the MI355X (two S = 17 sphere grids, 1,000 samples each): float64 worst 3.09e-08, fp32 worst 9.13e-08 (bound 1.24e-07)."""
    import dual_contour_ref
    from shapeclipper_amd import ops
    from shapeclipper_amd.utils import eval_3D
    level = _dev(np.stack([dual_contour_ref.sphere(17, 0.55, (0.1, -0.05, 0.2))[0], dual_contour_ref.sphere(17, 0.4, (0.0, 0.0, 0.0))[0]]))
    pts, _ = eval_3D.surface_points_device(level, -0.6, 0.6, 1000, seed=3)
    meshes = eval_3D.meshes_device(level, -0.6, 0.6)
    verts, faces = torch.cat([m[0] for m in meshes]).contiguous(), torch.cat([m[1] for m in meshes]).contiguous()
    v_count = torch.tensor([len(m[0]) for m in meshes], dtype=torch.int32, device=DEV)
    f_count = torch.tensor([len(m[1]) for m in meshes], dtype=torch.int32, device=DEV)
    got = ops.point_mesh_distance(pts.contiguous(), verts, faces, v_count, f_count)
    case = tuple(t.cpu().numpy() for t in (pts, verts, faces, v_count, f_count))
    exact = np.sqrt(ref.brute_exact(*case))
    dist = got.dist2.sqrt().cpu().numpy()
    print("samples on the mesh: float64 worst %.3g, fp32 worst %.3g" % (exact.max(), dist.max()))
    assert exact.max() < 1e-6 and dist.max() <= 4 * exact.max()
    _check(case, ref.point_mesh(*case), "surface samples")


# ---- 5. refusals and the raw C ABI -----------------------------------------------------------------------------------------------------------
def test_refusals(cases):
    from shapeclipper_amd import ops
    (pts, verts, faces, v_count, f_count), _ = cases["n65"]
    p, v, f, vc, fc = (_dev(x) for x in (pts, verts, faces, v_count, f_count))
    ops.point_mesh_distance(p, v, f, vc, fc)
    for bad in ((p.cpu(), v, f, vc, fc), (p, v.cpu(), f, vc, fc), (p, v, f.cpu(), vc, fc), (p, v, f, vc.cpu(), fc),
                (p.double(), v, f, vc, fc), (p, v.double(), f, vc, fc), (p, v, f.long(), vc, fc), (p, v, f, vc.long(), fc),
                (p, v, f, vc, fc.float()), (p[0], v, f, vc, fc), (p[..., :2].contiguous(), v, f, vc, fc), (p[:, :0], v, f, vc, fc),
                (p, v.view(-1), f, vc, fc), (p, v, f[:, :2].contiguous(), vc, fc), (p, v, f, vc.repeat(2), fc), (p, v, f, vc, fc[:0]),
                (p, v[:-1], f.clamp_max(len(v) - 2), vc, fc), (p, v, f[:-1], vc, fc), (p, v, f, vc + 1, fc), (p, v, f, vc, fc - 1),
                (p, v, f, -vc, fc), (p[:, ::2], v, f, vc, fc),
                (pts, v, f, vc, fc)):
        with pytest.raises(ValueError):
            ops.point_mesh_distance(*bad)
    for search in ("Grid", "", None, 0):
        with pytest.raises(ValueError, match="search"):
            ops.point_mesh_distance(p, v, f, vc, fc, search=search)
    for k, value in ((0, -1), (5, len(verts)), (len(faces) - 1, 1 << 30)):
        f_bad = f.clone()
        f_bad[k, k % 3] = value
        with pytest.raises(ValueError, match="outside its image's vertex range"):
            ops.point_mesh_distance(p, v, f_bad, vc, fc)
    # an index that is inside the packed array but outside ITS image's slice is refused too
    two = (torch.cat([p, p]), torch.cat([v, v]), torch.cat([f, f + len(verts)]), vc.repeat(2), fc.repeat(2))
    with pytest.raises(ValueError, match="outside its image's vertex range"):
        ops.point_mesh_distance(*two)
    none = ops.point_mesh_distance(p[:0], v[:0], f[:0], vc[:0], fc[:0])                 # no image: nothing is launched
    assert none.dist2.shape == (0, 65) and none.face.shape == (0, 65) and none.closest.shape == (0, 65, 3)


def test_raw_c_abi(cases):
    from shapeclipper_amd import _lib
    lib = _lib.load()
    (pts, verts, faces, v_count, f_count), want = cases["batch3"]
    B, N, V, F = pts.shape[0], pts.shape[1], len(verts), len(faces)
    nbytes = int(lib.sc_point_mesh_workspace_bytes(B, N, V, F))
    assert nbytes > 0 and lib.sc_point_mesh_workspace_bytes(0, N, V, F) == 0
    for args in ((65536, N, V, F), (B, 0, V, F), (B, N, -1, F), (B, N, V, -1), (B, N, V, (1 << 26) + 1), (40000, 40000, V, F)):
        assert lib.sc_point_mesh_workspace_bytes(*args) == -1
    p, st = _lib.ptr, _lib.stream
    t = [_dev(x) for x in (pts, verts, faces, v_count, f_count)]
    for fn in (lib.sc_point_mesh_distance, lib.sc_point_mesh_distance_brute):
        ws = torch.full((nbytes,), 0xA5, device=DEV, dtype=torch.uint8)                 # contents irrelevant on entry
        d = torch.full((B, N), -7.0, device=DEV)
        f = torch.full((B, N), -7, device=DEV, dtype=torch.int32)
        q = torch.full((B, N, 3), -7.0, device=DEV)
        assert fn(p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), B, N, V, F, p(ws), p(d), p(f), p(q), st()) == 0
        for name, g, w in zip(("dist2", "face", "closest"), (d, f, q), want):
            _same(g, w, "raw " + name)
        # a face index out of range is skipped, never read through: the same answer as the mesh without that face
        f_bad = t[2].clone()
        f_bad[3, 1] = V + 1000000
        f_bad[4, 0] = -5
        assert fn(p(t[0]), p(t[1]), p(f_bad), p(t[3]), p(t[4]), B, N, V, F, p(ws), p(d), p(f), p(q), st()) == 0
        bad_np = f_bad.cpu().numpy()
        for name, g, w in zip(("dist2", "face", "closest"), (d, f, q), ref.point_mesh(pts, verts, bad_np, v_count, f_count)):
            _same(g, w, "raw, skipped faces, " + name)
        # n_images <= 0 and refused arguments launch nothing: the outputs keep their fill
        d2, f2, q2 = torch.full_like(d, -7.0), torch.full_like(f, -7), torch.full_like(q, -7.0)
        for n_images in (0, -1):
            assert fn(p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), n_images, N, V, F, p(ws), p(d2), p(f2), p(q2), st()) == 0
        assert fn(p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), 65536, N, V, F, p(ws), p(d2), p(f2), p(q2), st()) == 1
        assert fn(p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), B, 0, V, F, p(ws), p(d2), p(f2), p(q2), st()) == 1
        assert fn(None, p(t[1]), p(t[2]), p(t[3]), p(t[4]), B, N, V, F, p(ws), p(d2), p(f2), p(q2), st()) == 1
        assert fn(p(t[0]), None, p(t[2]), p(t[3]), p(t[4]), B, N, V, F, p(ws), p(d2), p(f2), p(q2), st()) == 1
        assert fn(p(t[0]), p(t[1]), p(t[2]), p(t[3]), None, B, N, V, F, p(ws), p(d2), p(f2), p(q2), st()) == 1
        assert fn(p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), B, N, V, F, None, p(d2), p(f2), p(q2), st()) == 1
        assert fn(p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), B, N, V, F, p(ws), p(d2), None, p(q2), st()) == 1
        torch.cuda.synchronize()
        for x in (d2, f2, q2):
            assert bool((x == -7).all())


# ---- 6. the evaluation on the pix3d_mini tree ------------------------------------------------------------------------------------------------
MESH_FILES = ("completeness_mesh.txt", "cd_cat_mesh.txt", "f_score_mesh.txt")
DUAL_FILES = ("completeness_mesh_dual.txt", "cd_cat_mesh_dual.txt", "f_score_mesh_dual.txt")
NEW_KEYS = ("dist_comp_mesh", "cd_comp_mesh", "f_score_mesh", "face_mesh")
TREE_ARGS = ["--arch.enc_pretrained!", "--tb!", "--batch_size=2", "--data.pix3d.cat=chair,sofa", "--data.num_classes=2", "--data.num_workers=0",
             "--data.max_img_cat=2", "--eval.vox_res=16", "--eval.num_points=1000"]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from shapeclipper_amd.data import pix3d_mini
    root = str(tmp_path_factory.mktemp("pix3d_point_mesh") / "Pix3D")
    pix3d_mini.write_tree(root, n_per_cat=6, k_nearest=5, cat_key="chair,sofa", n_points=2000, seed=11)
    return root


def _opt(tree, output_root, extra=()):
    from shapeclipper_amd.utils import options
    o = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_point_mesh", "--output_root=%s" % output_root,
                                             "--data.pix3d.root=%s" % tree, *TREE_ARGS, *extra]), verbose=False)
    o.device, o.world_size, o.port = 0, 1, 0
    return o


def _runner(o):
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    from shapeclipper_amd.model.runner import Runner
    torch.manual_seed(0)
    r = Runner(o)
    r.load_dataset(o, eval_split="test")
    r.build_networks(o)
    r.graph.eval()
    return r


def _box_grid(o):
    """A level grid whose solid is the box |x| < .3, |y| < .2, |z| < .25, at get_dense_3D_grid's positions."""
    lo, hi = o.eval.range
    g = torch.linspace(lo, hi, o.eval.vox_res + 1, device=DEV)
    pts = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), dim=-1)
    return (pts.abs() - torch.tensor([0.3, 0.2, 0.25], device=DEV)).amax(dim=-1).contiguous()


def _sample_var(r, o, it=0):
    from shapeclipper_amd.utils.util import EasyDict as edict
    sample = r.test_data[it]
    batch = {k: ({kk: vv[None] for kk, vv in v.items()} if isinstance(v, dict) else torch.as_tensor(v)[None]) for k, v in sample.items()}
    o.H, o.W = o.eval.image_size
    with torch.no_grad():
        return r.evaluate_batch(o, edict(batch), 0, it, single_gpu=True)


def _files(o):
    """{relative name: bytes} of the .txt files of the output folder and of every per-sample file under dump/."""
    out = {}
    for folder in ("", "dump"):
        d = os.path.join(o.output_path, folder)
        for f in sorted(os.listdir(d)) if os.path.isdir(d) else []:
            if os.path.isfile(os.path.join(d, f)) and (folder or f.endswith(".txt")):
                out[os.path.join(folder, f)] = open(os.path.join(d, f), "rb").read()
    return out


def _check_formats(files, suffix, n, comp_not_above):
    lines = [l.split() for l in files["completeness_mesh%s.txt" % suffix].decode().splitlines()]
    raw = [l.split() for l in files["chamfer.txt"].decode().splitlines()]
    assert [int(l[0]) for l in lines] == [int(l[0]) for l in raw] == list(range(n))
    for l, c in zip(lines, raw):
        print("completeness_mesh%s.txt:" % suffix, " ".join(l))
        assert len(l) == 3 and all(len(x.split(".")[1]) == 8 for x in l[1:]) and l[1] == c[2]         # idx cd_comp cd_comp_mesh
        if comp_not_above:
            assert float(l[2]) <= float(l[1])
    cat, cat_raw = (files[f].decode().splitlines() for f in ("cd_cat_mesh%s.txt" % suffix, "cd_cat.txt"))
    assert cat[0] == cat_raw[0] == "CD     Acc    Comp   Count Cat" and len(cat) == len(cat_raw)
    for a, b in zip(cat[1:], cat_raw[1:]):
        a, b = a.split(), b.split()
        assert a[1] == b[1] and a[3:] == b[3:] and abs(float(a[0]) - (float(a[1]) + float(a[2])) / 2) <= 1.01e-4
        if comp_not_above:
            assert float(a[2]) <= float(b[2])
    fs, fs_raw = (files[f].decode().splitlines() for f in ("f_score_mesh%s.txt" % suffix, "f_score.txt"))
    assert len(fs) == len(fs_raw) == 6
    for a, b in zip(fs, fs_raw):
        assert a.split(":")[0] == b.split(":")[0] and a.startswith("F-score @ ") and len(a.split(": ")[1].split(".")[1]) == 4
        if comp_not_above:
            assert float(a.split(": ")[1]) >= float(b.split(": ")[1]) - 1e-4       # recall can only grow when no distance grows


def test_evaluation_writes_the_mesh_files_beside_the_raw_ones(tree, tmp_path, monkeypatch):
    from shapeclipper_amd import ops
    from shapeclipper_amd.utils import eval_3D
    o = _opt(tree, str(tmp_path))
    assert "mesh_dist" not in o.eval and "dual_mesh" not in o.eval
    r = _runner(o)
    grid = _box_grid(o)
    monkeypatch.setattr(eval_3D, "HAVE_MESHING", False)
    monkeypatch.setattr(eval_3D, "compute_level_grid", lambda opt, net, z, pts: grid[None].repeat(pts.shape[0], 1, 1, 1))
    n = len(r.test_data)
    assert n == 4
    net = r.graph.module.sdf_network

    # ---- off: without the key, and with the key set to false: the same bytes, nothing new ----
    raw_value = r.evaluate(o, ep=0)
    off = _files(o)
    assert {"chamfer.txt", "cd_cat.txt", "f_score.txt"} <= set(off) and not set(MESH_FILES + DUAL_FILES) & set(off)
    o.eval.mesh_dist = False
    assert r.evaluate(o, ep=0) == raw_value and _files(o) == off
    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net)
    assert not any(k in var for k in NEW_KEYS + ("dist_acc", "dist_comp", "mesh_dual"))
    raw = (var.cd_acc.clone(), var.cd_comp.clone(), var.f_score.clone(), var.dpc_pred.clone(), var.dpc.points.clone())

    # ---- on ----
    o.eval.mesh_dist = True
    assert r.evaluate(o, ep=0) == raw_value                             # the returned value is the raw one
    on = _files(o)
    for f, data in off.items():
        assert on[f] == data, f                                         # every existing output keeps its bytes
    assert sorted(set(on) - set(off)) == sorted(MESH_FILES)
    _check_formats(on, "", n, comp_not_above=True)

    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net)
    assert all(k in var for k in NEW_KEYS) and "cd_comp_dual" not in var and "mesh_dual" not in var
    for a, b in zip(raw, (var.cd_acc, var.cd_comp, var.f_score, var.dpc_pred, var.dpc.points)):
        assert torch.equal(a, b)                                        # the raw metrics are computed exactly as before
    assert var.dist_comp_mesh.shape == var.face_mesh.shape == (1, 2000) and var.cd_comp_mesh.shape == (1,) and var.f_score_mesh.shape == (1, 6)
    assert var.face_mesh.dtype == torch.int32 and bool((var.face_mesh >= 0).all())

    # ---- the same numbers from the ops chained by hand: the mesh through the maps the samples went through ----
    lo, hi = o.eval.range
    pts, _ = eval_3D.surface_points_device(var.level_vox, lo, hi, 1000, seed=int(var.idx[0]))
    rot = lambda Rm, P: (Rm @ P.permute(0, 2, 1)).permute(0, 2, 1).contiguous()
    flip = torch.tensor(eval_3D._FLIP_PRED, device=DEV).float()[None]
    centre, scale = eval_3D.normalize_pc_params(rot(flip, rot(var.pose[..., :3], pts)))
    (verts, faces), = eval_3D.meshes_device(var.level_vox, lo, hi)
    assert len(faces) > 100
    mapped = (((flip[0] @ (var.pose[0, :, :3].float() @ verts.t())).t() - centre[0]) / (scale[0] + 1e-7)).contiguous()
    i32 = dict(dtype=torch.int32, device=DEV)
    res = ops.point_mesh_distance(var.dpc.points.contiguous(), mapped, faces, torch.tensor([len(verts)], **i32), torch.tensor([len(faces)], **i32))
    assert torch.equal(res.dist2.sqrt().view(torch.int32), var.dist_comp_mesh.view(torch.int32)) and torch.equal(res.face, var.face_mesh)
    assert torch.equal(var.cd_comp_mesh, var.dist_comp_mesh.mean(dim=1))
    assert torch.equal(var.f_score_mesh, eval_3D.compute_fscore(var.dist_acc, var.dist_comp_mesh, o.eval.f_thresholds))
    assert on["completeness_mesh.txt"].decode().splitlines()[0] == "0 %.8f %.8f" % (float(var.cd_comp), float(var.cd_comp_mesh))
    # a sample lies on the mesh, so the mesh is never farther than the nearest sample -- up to how far the mapped samples are off the
    # mapped mesh in float64 (both went through fp32 maps), times 4, the margin of test_surface_samples_lie_on_the_indexed_mesh
    # (measured on the MI355X, sample 0: slack 3.79e-07; the largest dist_comp_mesh - dist_comp was -8.49e-07, i.e. no point is farther)
    case = tuple(t.cpu().numpy() for t in (var.dpc_pred, mapped, faces)) + (np.asarray([len(verts)], np.int32), np.asarray([len(faces)], np.int32))
    slack = 4 * float(np.sqrt(ref.brute_exact(*case)).max())
    excess = float((var.dist_comp_mesh - var.dist_comp).max())
    print("samples off the mapped mesh (float64) x 4 = %.3g; largest dist_comp_mesh - dist_comp = %.3g; cd_comp %.8f -> %.8f"
          % (slack, excess, float(var.cd_comp), float(var.cd_comp_mesh)))
    assert slack < 4e-6 and bool((var.dist_comp_mesh <= var.dist_comp + slack).all())      # for EVERY ground-truth point
    assert float(var.cd_comp_mesh) <= float(var.cd_comp)

    # ---- the sharded evaluation writes the same lines from its extra gather ----
    for f in MESH_FILES:
        os.remove(os.path.join(o.output_path, f))
    assert r.evaluate_sharded(o, ep=0) == pytest.approx(raw_value, rel=1e-5)
    sharded = _files(o)
    assert set(sharded) == set(on)
    if sharded["chamfer.txt"] == on["chamfer.txt"]:
        assert all(sharded[f] == on[f] for f in MESH_FILES)
    else:
        print("evaluate and evaluate_sharded differ on chamfer.txt: the mesh files are not compared")
    _check_formats(sharded, "", n, comp_not_above=True)

    # ---- the dual-contouring mesh: its files appear only together with --eval.dual_mesh, {idx}_mesh_dual.ply keeps its bytes ----
    o.eval.mesh_dist, o.eval.dual_mesh = False, True
    assert r.evaluate(o, ep=0) == raw_value
    dual_only = _files(o)
    ply = ["dump/%d_mesh_dual.ply" % i for i in range(n)]
    assert all(p in dual_only for p in ply) and not set(DUAL_FILES) & set(dual_only)
    o.eval.mesh_dist = True
    assert r.evaluate(o, ep=0) == raw_value
    both = _files(o)
    for f, data in dual_only.items():
        assert both[f] == data, f                                       # mesh_dual.ply among them: the mesh kept in var is the mesh dumped before
    assert sorted(set(both) - set(dual_only)) == sorted(DUAL_FILES) and all(both[f] == on[f] for f in MESH_FILES)
    _check_formats(both, "_dual", n, comp_not_above=False)
    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net)
    assert torch.equal(var.dist_comp_mesh.view(torch.int32), res.dist2.sqrt().view(torch.int32))
    (dv, df), = var.mesh_dual
    again, = eval_3D.meshes_dual(o, net, var.proj_latent_sdf, var.level_vox, 0.05)
    assert torch.equal(dv, again[0]) and torch.equal(df, again[1])
    dmapped = (((flip[0] @ (var.pose[0, :, :3].float() @ dv.t())).t() - centre[0]) / (scale[0] + 1e-7)).contiguous()
    dres = ops.point_mesh_distance(var.dpc.points.contiguous(), dmapped, df.contiguous(), torch.tensor([len(dv)], **i32), torch.tensor([len(df)], **i32))
    assert torch.equal(dres.dist2.sqrt().view(torch.int32), var.dist_comp_dual.view(torch.int32)) and torch.equal(dres.face, var.face_dual)
    assert both["completeness_mesh_dual.txt"].decode().splitlines()[0] == "0 %.8f %.8f" % (float(var.cd_comp), float(var.cd_comp_dual))
    for f in MESH_FILES + DUAL_FILES:
        os.remove(os.path.join(o.output_path, f))
    r.evaluate_sharded(o, ep=0)
    sharded = _files(o)
    assert set(sharded) == set(both)
    if sharded["chamfer.txt"] == both["chamfer.txt"]:
        assert all(sharded[f] == both[f] for f in MESH_FILES + DUAL_FILES)

    # ---- an empty mesh: one degenerate triangle at the first sample, the numbers of the raw completeness ----
    o.eval.dual_mesh = False
    monkeypatch.setattr(eval_3D, "compute_level_grid", lambda opt, net, z, pts: torch.ones_like(grid)[None].repeat(pts.shape[0], 1, 1, 1))
    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net)
    assert bool((var.face_mesh == 0).all()) and bool(torch.isfinite(var.dist_comp_mesh).all())
    assert torch.allclose(var.dist_comp_mesh, var.dist_comp, rtol=1e-5, atol=1e-7)          # every sample is the one point: the same distances

    # ---- vis_only skips it ----
    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net, vis_only=True)
    assert not any(k in var for k in NEW_KEYS)
