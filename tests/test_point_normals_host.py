"""k-NN PCA normals and normal consistency without a GPU: the numpy restatement (tests/point_normals_ref.py) has the geometry the issue
asks of it (sphere, cube, Jacobi against numpy.linalg.eigh, degenerate rows), the `--eval.normals*` options parse as documented, the
file formats are as documented, and the ops refuse bad arguments before anything reaches a device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import point_normals_ref as ref  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- the restatement's own checks ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere():
    p = ref.sphere(5, 2000)
    idx, dist = ref.knn(p, 16)
    return p, idx, dist


def test_knn_restatement_is_the_sorted_all_pairs_table(sphere):
    p, idx, dist = sphere
    assert idx.shape == (2000, 16) and idx.dtype == np.int32 and dist.dtype == np.float32
    assert np.array_equal(idx[:, 0], np.arange(2000)) and (dist[:, 0] == 0).all()          # the point itself comes first
    assert (np.diff(dist, axis=1) >= 0).all()
    d64 = ((p[:, None].astype(np.float64) - p[None].astype(np.float64)) ** 2).sum(-1)
    kth = np.sort(d64, axis=1)[:, 15]
    assert np.allclose(dist[:, 15], kth, rtol=1e-5, atol=0)
    for i in (0, 77, 1999):                                                                  # a row of the table, formed on its own
        keys = np.sort(ref.knn_keys(p, i))[:16]
        assert np.array_equal((keys & np.uint64(0xFFFFFFFF)).astype(np.int64), idx[i].astype(np.int64))
    # ties go to the lower index; a NaN distance sorts last
    q = np.float32([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [0, 0, 2]])
    i2, d2 = ref.knn(q, 5)
    assert i2[0].tolist() == [0, 1, 2, 3, 5] and d2[0].tolist() == [0, 1, 1, 1, 4]
    assert i2[4].tolist() == [0, 1, 2, 3, 4] and np.isnan(d2[4]).all()


def test_sphere_normals_are_radial(sphere):
    p, idx, _ = sphere
    n, var, lam = ref.normals(p, idx)
    r = p.astype(np.float64) / np.linalg.norm(p.astype(np.float64), axis=1, keepdims=True)
    cos = np.abs((n * r).sum(axis=1))
    gap = (lam[:, 1] - lam[:, 0]) / lam[:, 2]
    print("sphere: min |n . r| %.4f, mean %.4f, min eigen-gap %.3f, max variation %.4f" % (cos.min(), cos.mean(), gap.min(), var.max()))
    assert cos.min() >= 0.99 and cos.mean() >= 0.999
    assert gap.min() >= 1e-3
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() < 1e-7 and (var > 0).all() and (var < 1 / 3).all()
    big = np.take_along_axis(n, np.argmax(np.abs(n), axis=1)[:, None], axis=1)
    assert (big > 0).all()                                                                   # the sign rule


def test_cube_normals_are_the_face_axes():
    p, axis = ref.cube_surface(5, 3000)
    idx, _ = ref.knn(p, 16)
    n, _, _ = ref.normals(p, idx)
    other = np.abs(p).copy()
    other[np.arange(3000), axis] = 0
    inner = other.max(axis=1) < 0.3                                                          # more than 0.2 from every edge
    assert inner.sum() > 500
    along = np.abs(n[np.arange(3000), axis])[inner]
    print("cube: %d inner points, min |n_axis| %.9f" % (inner.sum(), along.min()))
    assert along.min() >= 1 - 1e-6


def test_eight_sweeps_agree_with_eigh(sphere):
    p, idx, _ = sphere
    dv, dl, kept = ref.jacobi_against_eigh(p, idx)
    print("sphere: Jacobi against eigh, worst |vector difference| %.3g, |eigenvalue difference| %.3g over %d points" % (dv, dl, kept))
    assert kept == 2000 and dv <= 1e-14 and dl <= 1e-16
    v = ref.volume(3, 1000)
    dv, dl, kept = ref.jacobi_against_eigh(v, ref.knn(v, 8)[0])
    print("volume: %.3g, %.3g over %d points" % (dv, dl, kept))
    assert kept >= 990 and dv <= 1e-12


def test_degenerate_rows_of_the_restatement():
    line = np.zeros((20, 3), np.float32)
    line[:, 0] = np.arange(20) * 0.25
    n, var, _ = ref.normals(line, ref.knn(line, 5)[0])
    assert not n.any() and not var.any()
    same = np.ones((20, 3), np.float32)
    n, var, _ = ref.normals(same, ref.knn(same, 5)[0])
    assert not n.any() and not var.any()
    v = ref.volume(1, 300)
    idx = ref.knn(v, 8)[0]
    want = ref.normals(v, idx)[0]
    bad = idx.copy()
    bad[5, 3] = 300                                                                          # an index outside the cloud
    v[9] = np.nan
    n, var, _ = ref.normals(v, bad)
    touched = (idx == 9).any(axis=1)
    touched[5] = True
    assert not n[touched].any() and not var[touched].any() and np.array_equal(n[~touched], want[~touched])


def test_normal_consistency_restatement():
    rng = np.random.default_rng(2)
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    n1, n2 = unit(rng.normal(size=(50, 3))), unit(rng.normal(size=(70, 3)))
    i1, i2 = rng.integers(0, 70, 50), rng.integers(0, 50, 70)
    acc, comp = ref.normal_consistency(n1, n2, i1, i2)
    assert 0 <= acc <= 1 and 0 <= comp <= 1
    assert abs(acc - np.mean([abs(float(np.dot(n1[i].astype(np.float64), n2[i1[i]].astype(np.float64)))) for i in range(50)])) < 1e-15
    a, c = ref.normal_consistency(n1, -n1, np.arange(50), np.arange(50))                     # unoriented: a flipped copy is consistent
    assert abs(a - 1) < 1e-7 and abs(c - 1) < 1e-7
    i1[3] = 70
    acc, comp2 = ref.normal_consistency(n1, n2, i1, i2)
    assert np.isnan(acc) and comp2 == comp


# ---- options ---------------------------------------------------------------------------------------------------------------------------
def _set(tmp_path, *extra):
    from shapeclipper_amd.utils import options
    return options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_normals_options",
                                                "--output_root=%s" % tmp_path, *extra]), verbose=False)


def test_normals_options_absent_means_off_and_defaults(tmp_path):
    from shapeclipper_amd.utils import options
    from shapeclipper_amd.utils.util import EasyDict as edict
    o = _set(tmp_path)
    assert options.normal_settings(o) is None
    assert "normals" not in o.eval and "normals_k" not in o.eval                            # nothing is written into the tree
    assert options.normal_settings(_set(tmp_path, "--eval.normals")) == 16
    assert options.normal_settings(_set(tmp_path, "--eval.normals", "--eval.normals_k=3")) == 3
    assert options.normal_settings(_set(tmp_path, "--eval.normals", "--eval.normals_k=32")) == 32
    assert options.normal_settings(_set(tmp_path, "--eval.normals!", "--eval.normals_k=8")) is None
    assert options.normal_settings(edict()) is None                                          # a tree built by hand, without an eval node
    assert not any("normals" in row.key for row in options.HIP_TABLE)                        # an evaluation setting, not a hip.* switch


@pytest.mark.parametrize("switch", [(), ("--eval.normals",)])
@pytest.mark.parametrize("bad", ["--eval.normals_k=2", "--eval.normals_k=33", "--eval.normals_k=true", "--eval.normals_k=16.0",
                                 "--eval.normals_k=many"])
def test_normals_options_refuse_bad_values_whether_or_not_the_switch_is_on(tmp_path, bad, switch):
    with pytest.raises(ValueError, match="eval.normals_k"):
        _set(tmp_path, bad, *switch)


def test_normals_switch_must_be_a_bool(tmp_path):
    with pytest.raises(ValueError, match="eval.normals must be a bool"):
        _set(tmp_path, "--eval.normals=2")


# ---- file formats ----------------------------------------------------------------------------------------------------------------------
def test_pointcloud_ply_with_normals(tmp_path):
    from shapeclipper_amd.utils import util_vis
    from shapeclipper_amd.utils.util import EasyDict as edict
    rng = np.random.default_rng(0)
    pred, gt = rng.normal(size=(1, 5, 3)).astype(np.float32), rng.normal(size=(1, 7, 3)).astype(np.float32)
    pn, gn = rng.normal(size=(1, 5, 3)).astype(np.float32), rng.normal(size=(1, 7, 3)).astype(np.float32)
    os.makedirs(tmp_path / "dump")
    opt = edict(output_path=str(tmp_path))
    util_vis.dump_pointclouds_compare(opt, [3], "pointclouds_normals", torch.tensor(pred), torch.tensor(gt), pred_normals=torch.tensor(pn),
                                      gt_normals=torch.tensor(gn))
    util_vis.dump_pointclouds_compare(opt, [3], "pointclouds_comp", pred, gt)
    data = open(tmp_path / "dump" / "3_pointclouds_normals.ply", "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    assert data[:end].decode("ascii").splitlines() == [
        "ply", "format binary_little_endian 1.0", "element vertex 12", "property float x", "property float y", "property float z",
        "property float nx", "property float ny", "property float nz", "property uchar red", "property uchar green", "property uchar blue",
        "end_header"]
    vdt = np.dtype([(k, "<f4") for k in ("x", "y", "z", "nx", "ny", "nz")] + [(k, "u1") for k in ("red", "green", "blue")])
    assert vdt.itemsize == 27 and len(data) == end + 27 * 12
    v = np.frombuffer(data, vdt, 12, end)
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), np.concatenate([pred[0], gt[0]]))
    assert np.array_equal(np.stack([v["nx"], v["ny"], v["nz"]], 1), np.concatenate([pn[0], gn[0]]))
    assert v["red"].tolist() == [255] * 5 + [0] * 7 and v["green"].tolist() == [0] * 5 + [255] * 7 and not v["blue"].any()
    # without normals the file is what it was: x y z red green blue, 15 bytes a vertex
    plain = open(tmp_path / "dump" / "3_pointclouds_comp.ply", "rb").read()
    assert b"nx" not in plain and len(plain) == plain.index(b"end_header\n") + len(b"end_header\n") + 15 * 12


def test_normal_consistency_files(tmp_path):
    from shapeclipper_amd.model import runner
    from shapeclipper_amd.utils.util import EasyDict as edict

    class Data:
        label2cat = {0: "chair", 1: "sofa"}

    class Stub:
        test_data = Data()

    opt = edict(output_path=str(tmp_path), data=edict(num_classes=2))
    rec = torch.tensor([[0, 0.5, 0.25, 0.375, 0, 0.75, 0.5, 0.625],
                        [1, 1.0, 0.5, 0.75, 1, 1.0, 1.0, 1.0],
                        [2, 0.25, 0.25, 0.25, 0, 0.5, 0.5, 0.5]], dtype=torch.float64)
    runner.Runner._write_normals(Stub(), opt, rec[:, :5])
    assert sorted(os.listdir(tmp_path)) == ["nc_cat.txt", "normal_consistency.txt"]
    assert open(tmp_path / "normal_consistency.txt").read() == "0 0.50000000 0.25000000 0.37500000\n1 1.00000000 0.50000000 0.75000000\n" \
                                                               "2 0.25000000 0.25000000 0.25000000\n"
    assert open(tmp_path / "nc_cat.txt").read() == "NC     Acc    Comp   Count Cat\n0.3123 0.3748 0.2499     2 chair\n0.7493 0.9990 0.4995     1 sofa\n"
    runner.Runner._write_normals(Stub(), opt, rec)
    assert sorted(os.listdir(tmp_path)) == ["nc_cat.txt", "nc_cat_icp.txt", "normal_consistency.txt", "normal_consistency_icp.txt"]
    assert open(tmp_path / "normal_consistency_icp.txt").read().splitlines()[0] == "0 0.75000000 0.50000000 0.62500000"
    assert open(tmp_path / "nc_cat_icp.txt").read().splitlines()[2] == "0.9990 0.9990 0.9990     1 sofa"
    var = edict(idx=torch.tensor([4]), nc_acc=torch.tensor([0.5], dtype=torch.float64), nc_comp=torch.tensor([1.0], dtype=torch.float64),
                nc=torch.tensor([0.75], dtype=torch.float64), category_label=torch.tensor([1]))
    assert runner._normal_records(var).tolist() == [[4, 0.5, 1.0, 0.75, 1]]
    assert runner.NC_LINE % (4, 0.5, 1.0, 0.75) == "4 0.50000000 1.00000000 0.75000000\n"


# ---- the ops' refusals that need no device ---------------------------------------------------------------------------------------------
def test_ops_refuse_before_touching_a_device():
    from shapeclipper_amd import ops
    p = torch.zeros(1, 40, 3)
    for bad in (2, 33, 16.0, True, None):
        with pytest.raises(ValueError, match="k in 3..32"):
            ops.knn_points(p, bad)
        with pytest.raises(ValueError, match="k in 3..32"):
            ops.point_normals(p, bad)
    with pytest.raises(ValueError):
        ops.knn_points(p[0], 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.knn_points(p, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.point_normals(p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.normal_consistency(p, p, torch.zeros(1, 40, dtype=torch.int32), torch.zeros(1, 40, dtype=torch.int32))
    assert ops.PointNormals._fields == ("normals", "variation", "idx", "dist")
