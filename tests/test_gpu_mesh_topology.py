"""ops.mesh_topology (csrc/mesh_topology.hip) on the GPU against the numpy restatement tests/mesh_topology_ref.py: every integer field,
the flags, face_component, the volume AND the area bit for bit.  The area was the open point -- same terms, same order, but a float64
square root on the device: the kernel takes the round-to-nearest one (__dsqrt_rn), test_area_term_of_single_faces_rounds_as_numpy
compares 4,096 single-face areas (one square root each, no sum) with numpy's bit for bit, and every case below agrees in the last
bit, so the relative 1e-12 the area was first held to is tightened to bit equality.  The two-rank run of evaluate.py is in
tests/test_zz_mesh_stats_two_ranks.py: tests that start other processes run behind the kernel tests.

Shapes: the hand-counted meshes of the host test (4 to 32 faces), a single face, a soup of 200 faces over 12 vertices (edges with many
faces, long probe chains at the smallest table), 600 faces (three chunks of the float64 sums), a batch with empty images, and level
grids of side 16 and 24 (a few thousand faces: more than one workgroup, more than one chunk).  The restatement of every case is
computed once per module and shared."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_topology_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MESHES = ref.meshes()
_REF = {}


def _ref(name, verts, faces):
    """The restatement of a named case, computed once."""
    if name not in _REF:
        _REF[name] = ref.mesh_topology(verts, faces)
    return _REF[name]


def _run(meshes, table_slots=None):
    """ops.mesh_topology of a list of (verts, faces) numpy meshes packed into one batch."""
    from shapeclipper_amd import ops
    verts = torch.as_tensor(np.concatenate([np.asarray(v, np.float32).reshape(-1, 3) for v, _ in meshes])).to(DEV)
    faces = torch.as_tensor(np.concatenate([np.asarray(f, np.int32).reshape(-1, 3) for _, f in meshes])).to(DEV)
    v_count = torch.tensor([len(v) for v, _ in meshes], dtype=torch.int64)
    f_count = torch.tensor([len(f) for _, f in meshes], dtype=torch.int64)
    return ops.mesh_topology(verts, faces, v_count, f_count, table_slots=table_slots)


def _check(got, wants, what):
    """Image b of the result `got` equals the restatement wants[b]."""
    first = 0
    for b, want in enumerate(wants):
        for k in ref.INT_FIELDS:
            assert got._asdict()[k].dtype == torch.int64
            assert int(got._asdict()[k][b]) == want[k], (what, b, k, int(got._asdict()[k][b]), want[k])
        for k in ref.FLAGS:
            assert got._asdict()[k].dtype == torch.bool and bool(got._asdict()[k][b]) == want[k], (what, b, k)
        n = len(want["face_component"])
        fc = got.face_component[first:first + n].cpu().numpy()
        assert fc.dtype == np.int32 and np.array_equal(fc, want["face_component"]), (what, b, "face_component")
        first += n
        volume, area = got.volume[b].cpu().numpy(), got.area[b].cpu().numpy()
        print("%s[%d]: F %d  volume %r (restated %r)  area %r (restated %r)%s" % (
            what, b, n, float(volume), float(want["volume"]), float(area), float(want["area"]),
            "" if area.view(np.int64) == want["area"].view(np.int64) else "  AREA BITS DIFFER"))
        assert volume.dtype == np.float64 and volume.view(np.int64) == want["volume"].view(np.int64), (what, b, "volume", volume, want["volume"])
        assert area.dtype == np.float64 and area.view(np.int64) == want["area"].view(np.int64), (what, b, "area", area, want["area"])
    assert first == got.face_component.shape[0]


def _bits(got):
    return [t.cpu().view(torch.int64 if t.dtype == torch.float64 else t.dtype).clone() for t in got]


# ---- level grids ---------------------------------------------------------------------------------------------------------------------
def _grid(S):
    g = np.arange(S, dtype=np.float64)
    return np.meshgrid(g, g, g, indexing="ij")


def _sphere(S, centre, r):
    x, y, z = _grid(S)
    return (np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - r).astype(np.float32)


def _torus_grid(S=24, R=6.5, r=2.6):
    x, y, z = _grid(S)
    c = (S - 1) / 2
    return (np.sqrt((np.sqrt((x - c) ** 2 + (y - c) ** 2) - R) ** 2 + (z - c) ** 2) - r).astype(np.float32)


LEVELS = {
    "sphere_inside": lambda: _sphere(16, (7.3, 7.6, 7.45), 5.2),
    "torus": _torus_grid,
    "two_spheres": lambda: np.minimum(_sphere(16, (4.0, 7.5, 7.5), 2.6), _sphere(16, (11.0, 7.5, 7.5), 2.6)),
    "sphere_cut": lambda: _sphere(16, (1.5, 7.5, 7.5), 4.0),
}
_MC = {}


def _marching_cubes(name):
    """(verts, faces, v_count, f_count) of ops.isosurface_mesh on the named level grid, once per module."""
    from shapeclipper_amd import ops
    if name not in _MC:
        _MC[name] = ops.isosurface_mesh(torch.as_tensor(LEVELS[name]())[None].to(DEV))
    return _MC[name]


def _mesh_case(name):
    from shapeclipper_amd import ops
    verts, faces, v_count, f_count = _marching_cubes(name)
    got = ops.mesh_topology(verts, faces, v_count, f_count)
    want = _ref("mc_" + name, verts.cpu().numpy(), faces.cpu().numpy())
    _check(got, [want], name)
    return got, want


# ---- the hand-counted meshes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MESHES))
def test_every_hand_counted_mesh_alone(name):
    verts, faces, expected = MESHES[name]
    got = _run([(verts, faces)])
    _check(got, [_ref(name, verts, faces)], name)
    for key, value in expected.items():
        assert got._asdict()[key][0].item() == value, (name, key)


def test_all_of_them_in_one_batch_with_empty_images():
    names = list(MESHES)
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    lonely = (np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int32))           # vertices without a face
    meshes = [MESHES[n][:2] for n in names[:4]] + [empty] + [MESHES[n][:2] for n in names[4:]] + [lonely, empty]
    wants = [_ref(n, *MESHES[n][:2]) for n in names[:4]] + [_ref("empty", *empty)] + [_ref(n, *MESHES[n][:2]) for n in names[4:]]
    wants += [_ref("lonely", *lonely), _ref("empty", *empty)]
    got = _run(meshes)
    _check(got, wants, "batch")
    for b in (4, len(meshes) - 1):
        assert [int(got._asdict()[k][b]) for k in ref.INT_FIELDS] == [0] * 12 + [-1]
        assert bool(got.watertight[b]) and bool(got.oriented[b]) and bool(got.manifold[b])
        assert float(got.area[b]) == 0.0 and float(got.volume[b]) == 0.0
    assert int(got.unreferenced_vertices[len(meshes) - 2]) == 3 and int(got.genus[len(meshes) - 2]) == -1


def test_soup_at_the_default_and_at_the_smallest_table():
    from shapeclipper_amd import ops
    verts, faces = ref.soup()
    want = _ref("soup", verts, faces)
    default = _run([(verts, faces)])
    _check(default, [want], "soup")
    assert ops.mesh_topology_slots(200) == 2048
    smallest = _run([(verts, faces)], table_slots=1024)                   # the smallest power of two above 3 F = 600
    _check(smallest, [want], "soup, 1024 slots")
    for a, b in zip(_bits(default), _bits(smallest)):
        assert torch.equal(a, b)
    assert want["nonmanifold_edges"] > 0 and want["degenerate_faces"] > 0


def test_one_face_and_three_chunks():
    one = (np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0]], np.float32), np.array([[0, 1, 2]], np.int32))
    got = _run([one])
    _check(got, [_ref("one", *one)], "one face")
    assert (int(got.edges[0]), int(got.boundary_edges[0]), int(got.euler[0]), float(got.area[0])) == (3, 3, 1, 2.0)
    rng = np.random.RandomState(5)
    verts = rng.uniform(-1, 1, (50, 3)).astype(np.float32)
    faces = np.stack([rng.permutation(50)[:3] for _ in range(600)]).astype(np.int32)
    _check(_run([(verts, faces), one]), [_ref("chunks", verts, faces), _ref("one", *one)], "600 faces")


def test_area_term_of_single_faces_rounds_as_numpy():
    """4,096 images of one triangle each, coordinates over eleven binades: an image's area is 0.0 + (0.0 + its one term), so the device's
    square root shows in every output on its own.  Bit for bit numpy's correctly rounded one; the volume term (a division) likewise."""
    from shapeclipper_amd import ops
    rng = np.random.RandomState(9)
    B = 4096
    verts = (rng.uniform(-1, 1, (B, 3, 3)) * 2.0 ** rng.randint(-5, 6, (B, 1, 1))).astype(np.float32)
    faces = np.tile(np.array([[0, 1, 2]], np.int32), (B, 1))
    got = ops.mesh_topology(torch.as_tensor(verts.reshape(-1, 3)).to(DEV), torch.as_tensor(faces).to(DEV), torch.full((B,), 3), torch.full((B,), 1))
    p = verts.astype(np.float64)
    zero = np.float64(0.0)
    want = np.array([[zero + (zero + t) for t in ref.face_terms(p[b, 0], p[b, 1], p[b, 2])] for b in range(B)])
    assert np.array_equal(got.area.cpu().numpy().view(np.int64), want[:, 0].view(np.int64))
    assert np.array_equal(got.volume.cpu().numpy().view(np.int64), want[:, 1].view(np.int64))
    assert got.boundary_edges.tolist() == [3] * B and got.components.tolist() == [1] * B


# ---- meshes of the project's own meshers -----------------------------------------------------------------------------------------------
def test_marching_cubes_sphere_inside_the_grid_is_a_closed_oriented_manifold():
    got, want = _mesh_case("sphere_inside")
    assert bool(got.watertight[0]) and bool(got.oriented[0]) and bool(got.manifold[0])
    assert (int(got.genus[0]), int(got.components[0]), int(got.euler[0])) == (0, 1, 2)
    assert int(got.faces[0]) > 2 * ref.CHUNK                             # several workgroups, several chunks
    sphere = 4 / 3 * np.pi * 5.2 ** 3
    assert 0.9 * sphere < abs(float(got.volume[0])) < sphere             # the chords of a convex surface lie inside it


def test_marching_cubes_torus_has_genus_one():
    got, _ = _mesh_case("torus")
    assert bool(got.watertight[0]) and bool(got.oriented[0]) and bool(got.manifold[0])
    assert (int(got.genus[0]), int(got.components[0]), int(got.euler[0])) == (1, 1, 0)


def test_two_separate_spheres_are_two_components():
    got, _ = _mesh_case("two_spheres")
    assert (int(got.components[0]), int(got.genus[0]), int(got.euler[0])) == (2, 0, 4)
    assert int(got.largest_component_faces[0]) * 2 == int(got.faces[0])
    assert min(got.face_component.tolist()) == 0 and len(set(got.face_component.tolist())) == 2


def test_sphere_cut_by_the_grid_boundary_has_boundary_edges():
    got, want = _mesh_case("sphere_cut")
    assert int(got.boundary_edges[0]) == want["boundary_edges"] > 0
    assert not bool(got.watertight[0]) and int(got.genus[0]) == -1
    assert bool(got.oriented[0]) and int(got.nonmanifold_edges[0]) == 0


def test_dual_contouring_mesh_of_the_inside_sphere_is_closed_with_genus_zero():
    from shapeclipper_amd import ops
    level = torch.as_tensor(LEVELS["sphere_inside"]())[None].to(DEV)
    verts = _marching_cubes("sphere_inside")[0]
    normals = torch.nn.functional.normalize(verts - torch.tensor([7.3, 7.6, 7.45], device=DEV), dim=1).contiguous()
    dverts, dfaces, dv_count, df_count = ops.dual_contour_mesh(level, normals)
    got = ops.mesh_topology(dverts, dfaces, dv_count, df_count)
    _check(got, [_ref("dual_sphere", dverts.cpu().numpy(), dfaces.cpu().numpy())], "dual sphere")
    assert bool(got.watertight[0]) and bool(got.oriented[0]) and bool(got.manifold[0])
    assert (int(got.genus[0]), int(got.components[0])) == (0, 1)


def test_permuting_the_faces_of_the_torus_leaves_the_integers():
    from shapeclipper_amd import ops
    verts, faces, v_count, f_count = _marching_cubes("torus")
    first = ops.mesh_topology(verts, faces, v_count, f_count)
    perm = torch.randperm(faces.shape[0], generator=torch.Generator().manual_seed(4)).to(DEV)
    again = ops.mesh_topology(verts, faces[perm].contiguous(), v_count, f_count)
    for k in ref.INT_FIELDS + ref.FLAGS:
        assert torch.equal(first._asdict()[k], again._asdict()[k]), k
    assert int(first.genus[0]) == 1


def test_two_runs_and_a_second_stream_give_the_same_bits():
    from shapeclipper_amd import ops
    verts, faces, v_count, f_count = _marching_cubes("torus")
    first = _bits(ops.mesh_topology(verts, faces, v_count, f_count))
    second = _bits(ops.mesh_topology(verts, faces, v_count, f_count))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        third = _bits(ops.mesh_topology(verts, faces, v_count, f_count))
    torch.cuda.synchronize()
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_refusals_leave_the_gpu_usable():
    from shapeclipper_amd import ops
    verts, faces = (torch.as_tensor(x).to(DEV) for x in MESHES["torus"][:2])
    vc, fc = torch.tensor([16]), torch.tensor([32])
    good = lambda: _check(ops.mesh_topology(verts, faces, vc, fc), [_ref("torus", *MESHES["torus"][:2])], "after a refusal")
    for slots in (64, 96, 100, 0, -128, 128.0, True, 1 << 31):          # 3 F = 96: not above it, not a power of two, not an int, too large
        with pytest.raises(ValueError, match="table_slots"):
            ops.mesh_topology(verts, faces, vc, fc, table_slots=slots)
    good()
    assert int(ops.mesh_topology(verts, faces, vc, fc, table_slots=128).genus[0]) == 1
    for args in ((verts.double(), faces, vc, fc), (verts, faces.long(), vc, fc), (verts, faces, vc.float(), fc), (verts.cpu(), faces, vc, fc),
                 (verts, faces.cpu(), vc, fc), (verts[:, :2], faces, vc, fc), (verts, faces.view(-1), vc, fc), (verts, faces, vc, fc[:0]),
                 (verts, faces, torch.tensor([15]), fc), (verts, faces, vc, torch.tensor([31])), (verts, faces, torch.tensor([17, -1]), torch.tensor([32, 0])),
                 ([[0.0, 0.0, 0.0]], faces, vc, fc)):
        with pytest.raises(ValueError):
            ops.mesh_topology(*args)
    good()
    for bad_index in (16, -1, 2 ** 31 - 1):                                 # outside [0, 16): flagged on the device, never dereferenced
        bad = faces.clone()
        bad[7, 1] = bad_index
        with pytest.raises(ValueError, match="vertex range"):
            ops.mesh_topology(verts, bad, vc, fc)
        good()
    two = torch.cat([verts, verts[:3]]), torch.cat([faces, faces[:1] * 0 + torch.tensor([[0, 1, 3]], dtype=torch.int32, device=DEV)])
    with pytest.raises(ValueError, match="vertex range"):                   # index 3 is in the batch's range, not in the second image's
        ops.mesh_topology(*two, torch.tensor([16, 3]), torch.tensor([32, 1]))
    good()


# ---- the evaluation's entry point ------------------------------------------------------------------------------------------------------
def test_eval_mesh_stats_fills_var_in_object_units():
    from shapeclipper_amd.utils import eval_3D
    from shapeclipper_amd.utils.util import EasyDict as edict
    lo, hi, S = -0.6, 0.6, 16
    opt = edict(eval=dict(range=[lo, hi], mesh_stats=True))
    level = torch.as_tensor(np.stack([LEVELS["sphere_inside"](), LEVELS["two_spheres"]()])).to(DEV)
    var = edict(level_vox=level)
    eval_3D.mesh_stats(opt, var)
    assert "mesh_stats_dual" not in var and len(var.mesh_packed) == 4
    stats = var.mesh_stats
    assert stats.genus.tolist() == [0, 0] and stats.components.tolist() == [1, 2] and stats.watertight.tolist() == [True, True]
    pitch = (hi - lo) / (S - 1)
    grid = _mesh_case("sphere_inside")[0]                                   # the same mesh in grid-index units
    assert float(stats.volume[0]) > 0
    assert abs(float(stats.volume[0]) / (float(grid.volume[0]) * pitch ** 3) - 1) < 1e-5
    assert abs(float(stats.area[0]) / (float(grid.area[0]) * pitch ** 2) - 1) < 1e-5
    verts, faces, v_count, f_count = var.mesh_packed
    world = (lo + verts * ((hi - lo) / (S - 1))).cpu().numpy()
    nv, nf = int(v_count[0]), int(f_count[0])
    want = ref.mesh_topology(world[:nv], faces[:nf].cpu().numpy())
    assert float(stats.volume[0]) == float(want["volume"]) and int(stats.edges[0]) == want["edges"]
    eval_3D.mesh_stats(opt, var)                                            # the packed mesh is taken from var the second time
    assert torch.equal(var.mesh_stats.volume, stats.volume)


# ---- the evaluation: --eval.mesh_stats on the pix3d_mini tree ----------------------------------------------------------------------------
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TREE_ARGS = ["--arch.enc_pretrained!", "--tb!", "--batch_size=2", "--data.pix3d.cat=chair,sofa", "--data.num_classes=2", "--data.num_workers=0",
             "--data.max_img_cat=2", "--eval.vox_res=16", "--eval.num_points=1000"]


def _files(o):
    """{relative name: bytes} of the .txt files of the output folder and of every per-sample file under dump/."""
    out = {}
    for folder in ("", "dump"):
        d = os.path.join(o.output_path, folder)
        for f in sorted(os.listdir(d)) if os.path.isdir(d) else []:
            if os.path.isfile(os.path.join(d, f)) and (folder or f.endswith(".txt")):
                out[os.path.join(folder, f)] = open(os.path.join(d, f), "rb").read()
    return out


def test_evaluation_writes_the_mesh_stats_files_beside_the_unchanged_ones(tmp_path, monkeypatch):
    """evaluate and evaluate_sharded on the pix3d_mini tree with a level grid whose solid is the box |x| < .3, |y| < .2, |z| < .25:
    off, no file of the switch; on, every other file keeps its bytes, every sample's line says closed, oriented, manifold, one
    component, genus 0, and the volume is the box's to the grid pitch; the vis_only pass (vis_{ep}/ of --hip.train_vis) fills var too;
    with --eval.dual_mesh the dual-contouring mesh is measured beside it."""
    from shapeclipper_amd.data import pix3d_mini
    from shapeclipper_amd.model import runner as runner_module
    from shapeclipper_amd.model.runner import Runner
    from shapeclipper_amd.utils import eval_3D, options
    from shapeclipper_amd.utils.util import EasyDict as edict
    tree = str(tmp_path / "Pix3D")
    pix3d_mini.write_tree(tree, n_per_cat=6, k_nearest=5, cat_key="chair,sofa", n_points=2000, seed=11)
    o = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_mesh_stats",
                                             "--output_root=%s" % (tmp_path / "out"), "--data.pix3d.root=%s" % tree, *TREE_ARGS]), verbose=False)
    o.device, o.world_size, o.port = 0, 1, 0
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    torch.manual_seed(0)
    r = Runner(o)
    r.load_dataset(o, eval_split="test")
    r.build_networks(o)
    r.graph.eval()
    lo, hi = o.eval.range
    g = torch.linspace(lo, hi, o.eval.vox_res + 1, device=DEV)
    pts = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), dim=-1)
    grid = (pts.abs() - torch.tensor([0.3, 0.2, 0.25], device=DEV)).amax(dim=-1).contiguous()
    monkeypatch.setattr(eval_3D, "HAVE_MESHING", False)
    monkeypatch.setattr(eval_3D, "compute_level_grid", lambda opt, net, z, pts: grid[None].repeat(pts.shape[0], 1, 1, 1))
    net = r.graph.module.sdf_network

    raw_value = r.evaluate(o, ep=0)
    off = _files(o)
    assert "chamfer.txt" in off and not [f for f in off if "mesh_stats" in f]
    o.eval.mesh_stats = False
    assert r.evaluate(o, ep=0) == raw_value and _files(o) == off

    o.eval.mesh_stats = True
    assert r.evaluate(o, ep=0) == raw_value
    on = _files(o)
    assert sorted(set(on) - set(off)) == ["mesh_stats.txt", "mesh_stats_cat.txt"] and all(on[f] == off[f] for f in off)
    lines = on["mesh_stats.txt"].decode().splitlines()
    print(on["mesh_stats.txt"].decode(), on["mesh_stats_cat.txt"].decode(), sep="\n")
    assert len(lines) == 4
    for it, line in enumerate(lines):
        f = line.split()
        assert len(f) == 19 and int(f[0]) == it and f[4:10] == ["0"] * 6                # no boundary, non-manifold, inconsistent, degenerate, unreferenced
        assert f[10] == "1" and f[11] == f[2] and f[12:17] == ["2", "0", "1", "1", "1"]     # one component, euler 2, genus 0, the three flags
        assert int(f[1]) - int(f[3]) + int(f[2]) == 2
        assert abs(float(f[18]) - 0.6 * 0.4 * 0.5) < 0.1 * 0.12 and float(f[17]) > 0        # the box's volume, in object units
    assert len(set(l.split(" ", 1)[1] for l in lines)) == 1                                 # the same grid for every sample
    cat = on["mesh_stats_cat.txt"].decode().splitlines()
    assert cat[0] == "Closed Comps   Genus  Count Cat" and len(cat) == 3
    assert all(c.split()[:3] == ["0.9995", "0.9995", "0.0000"] and c.split()[3] == "2" for c in cat[1:])
    for f in ("mesh_stats.txt", "mesh_stats_cat.txt"):
        os.remove(os.path.join(o.output_path, f))
    r.evaluate_sharded(o, ep=0)
    assert all(_files(o)[f] == on[f] for f in ("mesh_stats.txt", "mesh_stats_cat.txt", "chamfer.txt"))

    def sample_var(it=0):
        sample = r.test_data[it]
        batch = {k: ({kk: vv[None] for kk, vv in v.items()} if isinstance(v, dict) else torch.as_tensor(v)[None]) for k, v in sample.items()}
        o.H, o.W = o.eval.image_size
        with torch.no_grad():
            return r.evaluate_batch(o, edict(batch), 0, it, single_gpu=True)

    var = sample_var(1)                                                                     # the pass of vis_{ep}/ of --hip.train_vis
    eval_3D.eval_metrics(o, var, net, vis_only=True)
    assert "mesh_stats" in var and "mesh_stats_dual" not in var
    assert runner_module.mesh_stats_line(runner_module._mesh_stats_records(var)[0]).rstrip("\n") == lines[1]
    o.eval.mesh_stats = False
    var = sample_var(1)
    eval_3D.eval_metrics(o, var, net, vis_only=True)
    assert "mesh_stats" not in var and "mesh_packed" not in var

    o.eval.mesh_stats, o.eval.dual_mesh = True, True                                        # the dual-contouring mesh beside it
    var = sample_var(1)
    eval_3D.eval_metrics(o, var, net)
    assert runner_module._mesh_stats_rows(var).shape == (1, 38) and "mesh_dual" in var
    dual = var.mesh_stats_dual
    print("dual:", runner_module.mesh_stats_line(runner_module._mesh_stats_rows(var)[0], 20))
    dverts, dfaces, dv_count, df_count = var.mesh_dual_packed
    want = ref.mesh_topology((lo + dverts * ((hi - lo) / (grid.shape[0] - 1))).cpu().numpy(), dfaces.cpu().numpy())
    for k in ref.INT_FIELDS + ref.FLAGS:
        assert dual[k][0].item() == want[k], k
    assert float(dual.volume[0]) == float(want["volume"]) and float(dual.area[0]) == float(want["area"])
    assert int(dual.components[0]) == 1 and int(dual.boundary_edges[0]) == 0
