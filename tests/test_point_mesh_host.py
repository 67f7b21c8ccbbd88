"""Host checks of the point-to-mesh distance: the numpy restatement (tests/point_mesh_ref.py) against analytic cases and against float64 on
the inputs of the GPU tests, eval_3D.normalize_pc_params, options.mesh_dist_settings and the runner's writers.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import point_mesh_ref as ref  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32
A, B, C = (np.asarray(v, f32) for v in ([0, 0, 0], [2, 0, 0], [0, 2, 0]))


def _one(p, a=A, b=B, c=C):
    d, q, region = ref.pair(np.asarray(p, f32), a, b, c)
    return float(d), q, int(region)


# ---- the walk on one triangle ---------------------------------------------------------------------------------------------------------------
def test_a_point_above_the_interior_gives_the_plane_distance():
    d, q, region = _one([0.5, 0.25, 3.0])
    assert region == 6 and d == 9.0 and np.array_equal(q, np.asarray([0.5, 0.25, 0], f32))
    d, q, region = _one([0.5, 0.5, -0.125])
    assert region == 6 and d == 0.015625 and np.array_equal(q, np.asarray([0.5, 0.5, 0], f32))


@pytest.mark.parametrize("p, vertex, region", [([-1, -2, 1], A, 0), ([4, -1, 0.5], B, 1), ([-0.5, 3, -1], C, 3)])
def test_a_point_in_each_vertex_region(p, vertex, region):
    d, q, got = _one(p)
    assert got == region and np.array_equal(q, vertex) and d == float(((np.asarray(p, f32) - vertex) ** 2).sum())


@pytest.mark.parametrize("p, q_want, region", [([1, -3, 0], [1, 0, 0], 2), ([-2, 0.5, 1], [0, 0.5, 0], 4), ([2, 2, 0.5], [1, 1, 0], 5)])
def test_a_point_in_each_edge_region(p, q_want, region):
    d, q, got = _one(p)
    assert got == region and np.array_equal(q, np.asarray(q_want, f32)) and d == float(((np.asarray(p, f32) - q) ** 2).sum())


def test_a_point_on_a_vertex_or_an_edge_gives_zero_and_the_lowest_face():
    """Four triangles of a fan share the vertex (0,0,0); faces 1 and 2 share the edge to (0,2,0)."""
    verts = np.asarray([[0, 0, 0], [2, 0, 0], [0, 2, 0], [-2, 0, 0], [0, -2, 0]], f32)
    faces = np.asarray([[0, 4, 1], [0, 1, 2], [0, 2, 3], [0, 3, 4]], np.int32)
    pts = np.asarray([[0, 0, 0], [0, 1, 0], [0, 2, 0], [1, 0, 0], [-1, 0, 0], [1, 1, 0]], f32)
    d, f, q = ref.brute(pts, verts, faces)
    assert np.array_equal(d, np.zeros(6, f32)) and np.array_equal(q, pts)
    assert f.tolist() == [0, 1, 1, 0, 2, 1]
    # the same fan listed backwards: the minimum is the same, the index is again the lowest that attains it
    d2, f2, _ = ref.brute(pts, verts, faces[::-1])
    assert np.array_equal(d2, d) and f2.tolist() == [0, 1, 1, 2, 0, 2]


def test_a_point_triangle_acts_as_a_point():
    p = np.asarray([[0.3, -0.2, 0.9], [1, 1, 1], [0.25, 0.5, 0.125]], f32)
    a = np.asarray([0.25, 0.5, 0.125], f32)
    d, q, region = ref.pair(p, a, a, a)
    assert np.array_equal(q, np.broadcast_to(a, (3, 3))) and region.tolist() == [0, 0, 0]
    r = p - a
    assert np.array_equal(d, (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]) and d[2] == 0


def test_a_collinear_triangle_acts_as_a_segment():
    """(0,0,0), (1,0,0), (3,0,0) and its permutations: the segment from x = 0 to x = 3.  No NaN from the 0 / 0 of the textbook walk."""
    corners = [np.asarray(v, f32) for v in ([0, 0, 0], [1, 0, 0], [3, 0, 0])]
    pts = np.asarray([[-1, 1, 0], [0.5, 2, 0], [2, 0, -1], [2.5, 0, 0], [4, 0, 3], [1, 0, 0]], f32)
    want = np.asarray([2, 4, 1, 0, 10, 0], f32)
    for order in ((0, 1, 2), (1, 0, 2), (2, 1, 0), (1, 2, 0), (0, 2, 1), (2, 0, 1), (0, 0, 2), (0, 2, 2), (2, 0, 0)):
        d, q, _ = ref.pair(pts, *(corners[k] for k in order))
        assert np.array_equal(d, want), order
        assert not np.isnan(q).any() and np.array_equal(q[:, 1:], np.zeros((6, 2), f32))


def test_a_thin_sliver_is_taken_as_its_edges_and_an_ordinary_triangle_is_not():
    a, b = np.asarray([0, 0, 0], f32), np.asarray([1, 0, 0], f32)
    p = np.asarray([0.5, 0.0005, 0.25], f32)
    _, _, region = ref.pair(p, a, b, np.asarray([0.5, 0.001, 0], f32))          # sin^2 at a = 4e-6 < FLAT
    assert int(region) == 7
    d, _, region = ref.pair(p, a, b, np.asarray([0.5, 0.01, 0], f32))           # sin^2 at a = 4e-4
    assert int(region) == 6 and abs(float(d) - 0.0625) < 1e-8


def test_nan_never_wins_and_bad_faces_are_skipped():
    verts = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 1], [0, 0, 5], [1, 0, 5], [0, 1, 5]], f32)
    pts = np.asarray([[0.25, 0.25, 1.0], [np.inf, 0, 0]], f32)
    d, f, q = ref.brute(pts, verts, np.asarray([[3, 3, 3], [4, 5, 6], [0, 1, 7], [-1, 1, 2], [0, 1, 2]], np.int32))
    assert d[0] == 1 and f[0] == 4 and np.array_equal(q[0], np.asarray([0.25, 0.25, 0], f32))
    assert np.isnan(d[1]) and f[1] == -1 and np.isnan(q[1]).all()
    d, f, q = ref.brute(pts[:1], verts, np.asarray([[3, 3, 3], [0, 1, 9]], np.int32))     # a NaN triangle and a skipped one: no winner
    assert np.isposinf(d[0]) and f[0] == -1 and not q.any()
    d, f, q = ref.brute(pts[:1], verts, np.zeros((0, 3), np.int32))
    assert np.isposinf(d[0]) and f[0] == -1 and not q.any()


# ---- fp32 against float64 on the inputs of the GPU tests ---------------------------------------------------------------------------------------
def test_fp32_restatement_against_float64_on_the_gpu_tests_inputs():
    """Largest |sqrt(d fp32) - sqrt(d float64)| of a query's minimum, the float64 side being point_mesh_ref.brute_exact.  Measured here:
    sphere 5.35e-07 (far queries, distance up to 9), batch3 1.73e-07, huge 1.45e-07, flat 2.99e-08, n1 2.16e-08, n65 2.30e-08,
    f1 2.54e-07, degenerate 1.16e-06 (the slivers' width).  The bounds are 4 times the worst of the ordinary meshes and 4 times the
    degenerate mesh's own figure."""
    worst = {}
    for name, case in ref.cases().items():
        d32, f32_, q32 = ref.point_mesh(*case)
        exact = ref.brute_exact(*case)
        ok = np.isfinite(exact)
        assert np.array_equal(ok, np.isfinite(d32)) and not np.isnan(d32).any(), name
        worst[name] = float(np.abs(np.sqrt(d32[ok].astype(np.float64)) - np.sqrt(exact[ok])).max()) if ok.any() else 0.0
        # the closest point is on the winning face and at the distance reported
        pts, verts, faces, v_count, f_count = case
        r = pts[ok].astype(np.float64) - q32[ok].astype(np.float64)
        assert np.abs(np.sqrt((r * r).sum(-1)) - np.sqrt(d32[ok].astype(np.float64))).max() < 1e-6, name
    print("fp32 against float64:", "  ".join("%s %.3g" % kv for kv in worst.items()))
    assert worst.pop("degenerate") <= ref.FP32_VS_EXACT_BOUND_DEGENERATE
    assert max(worst.values()) <= ref.FP32_VS_EXACT_BOUND


def test_float64_twin_agrees_with_the_other_route_on_ordinary_triangles():
    for name in ("sphere", "huge", "flat", "f1"):
        case = ref.cases()[name]
        d64, _, _ = ref.point_mesh(*case, dtype=np.float64)
        assert np.abs(np.sqrt(d64) - np.sqrt(ref.brute_exact(*case))).max() < 1e-12, name


def test_generators_are_what_the_gpu_tests_say():
    cs = ref.cases()
    assert 300 <= len(cs["sphere"][2]) <= 1000 and cs["sphere"][0].shape == (1, 2000, 3)
    assert cs["batch3"][4].tolist() == [len(cs["sphere"][2]), 0, 201] and cs["batch3"][0].shape[0] == 3
    assert len(cs["huge"][2]) == 501 and cs["n1"][0].shape[1] == 1 and cs["n65"][0].shape[1] == 65 and len(cs["f1"][2]) == 1
    assert np.ptp(cs["flat"][1][:, 2]) == 0
    v, f = cs["degenerate"][1], cs["degenerate"][2]
    assert (f[:50] == f[0]).all() and (f[50:70, 0] == f[50:70, 1]).all() and (f[50:70, 1] == f[50:70, 2]).all()
    for pts, verts, faces, v_count, f_count in cs.values():
        assert pts.dtype == verts.dtype == f32 and faces.dtype == v_count.dtype == f_count.dtype == np.int32
        assert v_count.sum() == len(verts) and f_count.sum() == len(faces)


# ---- the evaluation's host side --------------------------------------------------------------------------------------------------------------
def test_normalize_pc_params_reproduce_normalize_pc_bit_for_bit():
    from shapeclipper_amd.utils import eval_3D
    torch.manual_seed(3)
    for pc in (torch.randn(3, 500, 3), torch.randn(1, 7, 3) * 40 + 5, torch.rand(2, 1000, 3) * torch.tensor([0.1, 3.0, 1.0])):
        before = pc.clone()
        centre, scale = eval_3D.normalize_pc_params(pc)
        assert centre.shape == (pc.shape[0], 1, 3) and scale.shape == (pc.shape[0], 1, 1) and torch.equal(pc, before)
        assert torch.equal(((pc - centre) / (scale + 1.e-7)).view(torch.int32), eval_3D.normalize_pc(pc).view(torch.int32))


def _set(tmp_path, *extra):
    from shapeclipper_amd.utils import options
    return options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_mesh_dist",
                                               "--output_root=%s" % tmp_path, *extra]), verbose=False)


def test_mesh_dist_settings(tmp_path):
    from shapeclipper_amd.utils import options
    from shapeclipper_amd.utils.util import EasyDict as edict
    o = _set(tmp_path)
    assert "mesh_dist" not in o.eval and options.mesh_dist_settings(o) is None            # absent means off
    assert options.mesh_dist_settings(_set(tmp_path, "--eval.mesh_dist")) is True
    assert options.mesh_dist_settings(_set(tmp_path, "--eval.mesh_dist!")) is None
    assert options.mesh_dist_settings(edict()) is None                                    # a tree built by hand, without an eval node
    for bad in ("--eval.mesh_dist=1", "--eval.mesh_dist=2", "--eval.mesh_dist=0.5", "--eval.mesh_dist=grid"):
        with pytest.raises(ValueError, match="eval.mesh_dist must be a bool"):
            _set(tmp_path, bad)
    for bad in (1, 0, "true", None, 1.0):
        o.eval.mesh_dist = bad
        with pytest.raises(ValueError, match="eval.mesh_dist must be a bool"):
            options.mesh_dist_settings(o)


def test_the_writers_line_formats(tmp_path):
    from shapeclipper_amd.model import runner
    from shapeclipper_amd.utils.util import EasyDict as edict
    assert runner.MESH_LINE % (7, 0.0123456789, 0.5) == "7 0.01234568 0.50000000\n"
    opt = edict(output_path=str(tmp_path), data=edict(num_classes=2), eval=edict(f_thresholds=[0.005, 0.01, 0.02, 0.05, 0.1, 0.2]))
    import types
    fake = types.SimpleNamespace(test_data=types.SimpleNamespace(label2cat={0: "chair", 1: "sofa"}))
    T = 6
    #        idx  acc   comp  comp_mesh  f_score_mesh x 6                      cat  comp_dual  f_score_dual x 6
    rows = [[0, 0.10, 0.20, 0.15, 0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0, 0.25, 1.0, 0.9, 0.8, 0.7, 0.6, 0.5],
            [1, 0.30, 0.40, 0.35, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 1, 0.45, 0.0, 0.1, 0.2, 0.3, 0.4, 0.5],
            [2, 0.50, 0.60, 0.55, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0, 0.65, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5]]
    recs = torch.tensor(rows, dtype=torch.float64)
    read = lambda f: open(os.path.join(str(tmp_path), f)).read()
    runner.Runner._write_mesh(fake, opt, recs[:, :5 + T])
    assert sorted(os.listdir(str(tmp_path))) == ["cd_cat_mesh.txt", "completeness_mesh.txt", "f_score_mesh.txt"]
    assert read("completeness_mesh.txt") == "0 0.20000000 0.15000000\n1 0.40000000 0.35000000\n2 0.60000000 0.55000000\n"
    assert read("cd_cat_mesh.txt") == ("CD     Acc    Comp   Count Cat\n0.3248 0.2999 0.3498     2 chair\n0.3247 0.2997 0.3497     1 sofa\n")
    assert read("f_score_mesh.txt") == "".join("F-score @ %.2f: %.4f\n" % (th * 100, v) for th, v in
                                               zip(opt.eval.f_thresholds, (0.2, 0.3, 0.4, 0.5, 0.6, 0.7)))
    os.remove(os.path.join(str(tmp_path), "completeness_mesh.txt"))
    runner.Runner._write_mesh(fake, opt, recs, per_sample=False)              # evaluate: dump_results wrote the per-sample lines
    assert sorted(os.listdir(str(tmp_path))) == ["cd_cat_mesh.txt", "cd_cat_mesh_dual.txt", "f_score_mesh.txt", "f_score_mesh_dual.txt"]
    assert read("cd_cat_mesh_dual.txt") == ("CD     Acc    Comp   Count Cat\n0.3748 0.2999 0.4498     2 chair\n0.3746 0.2997 0.4496     1 sofa\n")
    assert read("f_score_mesh_dual.txt").splitlines()[0] == "F-score @ 0.50: 0.5000"
    runner.Runner._write_mesh(fake, opt, recs)
    assert read("completeness_mesh_dual.txt") == "0 0.20000000 0.25000000\n1 0.40000000 0.45000000\n2 0.60000000 0.65000000\n"
    # the record of a batch: one row per sample, the dual columns only when they exist
    var = edict(idx=torch.tensor([4, 5]), cd_acc=torch.tensor([0.1, 0.2]), cd_comp=torch.tensor([0.3, 0.4]), cd_comp_mesh=torch.tensor([0.25, 0.35]),
                f_score_mesh=torch.arange(12.).view(2, 6), category_label=torch.tensor([1, 0]))
    rec = runner._mesh_records(var)
    assert rec.shape == (2, 11) and rec.dtype == torch.float64 and rec[:, 0].tolist() == [4, 5] and rec[:, 10].tolist() == [1, 0]
    assert rec[1, 4:10].tolist() == [6, 7, 8, 9, 10, 11] and rec[0, 3].item() == float(torch.tensor(0.25))
    var.cd_comp_dual, var.f_score_dual = torch.tensor([0.5, 0.6]), torch.ones(2, 6)
    assert runner._mesh_records(var).shape == (2, 18)
