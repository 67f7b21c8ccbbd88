"""The volumetric IoU without a GPU: the numpy restatement tests/voxel_iou_ref.py of sc_voxel_frame / sc_voxel_solid / sc_voxel_iou against
scipy.ndimage's binary_erosion(binary_fill_holes(binary_dilation(shell))), the leak that the closing is there for, the frame,
options.iou_settings, the refusals of the ops that are made before the device is looked at, and the writers of iou.txt / iou_cat.txt."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_iou_ref as ref  # noqa: E402

F = np.float32


@pytest.fixture(scope="module")
def pairs():
    return {name: ref.shape_pair(name) for name in ref.SHAPES}


# ---- the restatement against scipy.ndimage ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [8, 32, 33, 64])
@pytest.mark.parametrize("name", ["sphere", "torus", "box", "chair"])
def test_restatement_equals_scipy_bit_for_bit(pairs, name, res):
    """Both clouds of the pair, close = 0, 1 and 2: the packed solid of the Jacobi sweeps is scipy's, voxel for voxel; it holds the
    shell; the counts are the popcounts."""
    a, b = pairs[name]
    for close in (0, 1, 2):
        origin, pitch = ref.frame_one(a, b, res, close)
        for cloud in (a, b):
            s = ref.solid_one(cloud, origin, pitch, res, close)
            shell = ref.shell_volume(cloud, origin, pitch, res, close)
            want = ref.scipy_solid(shell, close)
            got = ref.unpack(s.bits)
            assert np.array_equal(got, want), (name, res, close, int((got != want).sum()))
            assert not (shell & ~got).any()                                         # the closing is extensive
            assert s.shell_voxels == int(shell.sum()) > 0 and s.solid_voxels == int(want.sum()) >= s.shell_voxels
            assert s.sweeps >= 1 and np.array_equal(ref.pack(got), s.bits)
            m = close + 1
            assert not got[:m].any() and not got[-m:].any() and not got[:, :m].any() and not got[:, -m:].any()
            assert not got[:, :, :m].any() and not got[:, :, -m:].any()             # m empty layers on every side


def test_the_leak_and_the_closing():
    """A seeded box surface (half extents 0.5, 0.3, 0.2) of 8,192 points at R = 32, in the frame of the 100,000-point cloud of the same
    box.  close = 0: the shell has pinholes, the exterior gets in, nothing is filled -- the solid IS the shell.  close = 1: the solid is
    that of the 100,000-point cloud to within 1 % of its voxels.  (This seed: shell 2,087 = solid at close 0, IoU with the dense solid
    0.28; at close 1 both solids are the full box of 6,048 voxels.)"""
    sparse, dense = ref.box_surface(8192, seed=0), ref.box_surface(100000, seed=5)
    assert len(sparse) == 8192
    origin, pitch = ref.frame_one(dense, dense, 32, 0)
    s0, d0 = ref.solid_one(sparse, origin, pitch, 32, 0), ref.solid_one(dense, origin, pitch, 32, 0)
    print("close 0: sparse shell %d solid %d, dense shell %d solid %d" % (s0.shell_voxels, s0.solid_voxels, d0.shell_voxels, d0.solid_voxels))
    assert s0.solid_voxels == s0.shell_voxels
    assert d0.solid_voxels > 3 * d0.shell_voxels                                    # the dense cloud does fill
    origin, pitch = ref.frame_one(dense, dense, 32, 1)
    s1, d1 = ref.solid_one(sparse, origin, pitch, 32, 1), ref.solid_one(dense, origin, pitch, 32, 1)
    differ = ref.popcount(s1.bits ^ d1.bits)
    print("close 1: sparse solid %d, dense solid %d, %d voxels differ" % (s1.solid_voxels, d1.solid_voxels, differ))
    assert differ <= 0.01 * d1.solid_voxels
    assert s1.solid_voxels > 3 * s1.shell_voxels                                    # closed, the sparse cloud fills too


def test_serpentine_needs_hundreds_of_sweeps():
    pts, origin, pitch = ref.serpentine(32)
    s = ref.solid_one(pts, origin, pitch, 32, 0)
    assert s.sweeps > 300 and s.solid_voxels == s.shell_voxels == len(pts)           # the exterior reaches all of the inside
    assert np.array_equal(ref.unpack(s.bits), ref.scipy_solid(ref.shell_volume(pts, origin, pitch, 32, 0), 0))
    shut = pts[~((pts[:, 0] == 1.5) & (pts[:, 1] == 2.5))]                           # without the hole's column the box is closed ...
    shut = np.concatenate([shut, np.array([[1.5, 2.5, z + 0.5] for z in range(1, 31)], F)])
    s = ref.solid_one(shut, origin, pitch, 32, 0)
    assert s.solid_voxels == 30 ** 3 and s.sweeps == 1                               # ... and fills


# ---- the frame ---------------------------------------------------------------------------------------------------------------------------
def test_frame():
    a, b = ref.shape_pair("chair", n=5000)
    for res, close in ((8, 2), (32, 1), (33, 0), (64, 2)):
        m = close + 1
        origin, pitch = ref.frame_one(a, b, res, close)
        assert origin.dtype == F and origin.shape == (3,) and isinstance(pitch, F)
        both = np.concatenate([a, b])
        lo, hi = both.min(0), both.max(0)
        assert pitch == F((hi - lo).max() / F(res - 2 * m))
        for cloud in (a, b):
            i = ref.shell_indices(cloud, origin, pitch, res, close)
            assert i.min() >= m and i.max() <= res - 1 - m
        i = ref.shell_indices(both, origin, pitch, res, close)
        assert i.max(0).max() - i.min(0).min() >= res - 2 * m - 1                    # the longest axis spans the interior
    p = np.tile(np.array([[0.3, -0.2, 0.1]], F), (7, 1))
    origin, pitch = ref.frame_one(p, p, 32, 1)
    assert pitch == F(1.0) and np.array_equal(origin, p[0] - F(16.0))               # coincident clouds
    s = ref.solid_one(p, origin, pitch, 32, 1)
    assert s.shell_voxels == 1 and s.solid_voxels == 1 and ref.unpack(s.bits)[16, 16, 16]
    assert ref.pair_iou(p, p, 32, 1)[:3] == (1.0, 1, 1)


def test_non_finite_input():
    a, b = ref.shape_pair("sphere", n=2000)
    origin, pitch = ref.frame_one(a, b, 32, 1)
    clean = ref.solid_one(a, origin, pitch, 32, 1)
    dirty = a.copy()
    dirty[5] = [np.nan, 0.0, 0.0]
    dirty[9] = [0.0, np.inf, 0.0]
    dirty[11] = [0.0, 0.0, -np.inf]
    kept = np.delete(a, [5, 9, 11], axis=0)
    s = ref.solid_one(dirty, origin, pitch, 32, 1)                                   # a row that is not finite is skipped
    assert np.array_equal(s.bits, ref.solid_one(kept, origin, pitch, 32, 1).bits) and s.shell_voxels <= clean.shell_voxels
    o, p = ref.frame_one(dirty, b, 32, 1)                                            # its pair has no frame
    assert np.isnan(o).all() and np.isnan(p)
    assert o.view(np.uint32).tolist() == [0x7fc00000] * 3
    s = ref.solid_one(a, o, p, 32, 1)
    assert s.shell_voxels == 0 and s.solid_voxels == 0 and not s.bits.any()
    iou, inter, union, _, _ = ref.pair_iou(dirty, b, 32, 1)
    assert np.isnan(iou) and inter == 0 and union == 0
    assert ref.iou_value(0, 0) == 1.0 and ref.iou_value(3, 4) == 0.75                # an empty union alone counts as 1
    huge = (a.astype(np.float64) * 6e38).astype(F)                               # finite, but hi - lo overflows
    o, p = ref.frame_one(huge, huge, 32, 1)
    assert not np.isfinite(p) and ref.solid_one(huge, o, p, 32, 1).solid_voxels == 0


def test_popcounts():
    rng = np.random.RandomState(0)
    a = rng.randint(0, 2, (3, 8, 8, 8)).astype(bool)
    b = rng.randint(0, 2, (3, 8, 8, 8)).astype(bool)
    b[2] = a[2] = False
    wa = np.stack([ref.pack(v) for v in a]).view(np.int64)
    wb = np.stack([ref.pack(v) for v in b]).view(np.int64)
    inter, union = ref.voxel_iou(wa, wb)
    assert inter.tolist() == [(x & y).sum() for x, y in zip(a, b)] and union.tolist() == [(x | y).sum() for x, y in zip(a, b)]
    assert ref.iou_value(inter, union)[2] == 1.0
    full = np.ones((64, 64, 64), bool)
    assert ref.popcount(ref.pack(full)) == 64 ** 3 and np.array_equal(ref.unpack(ref.pack(full)), full)


# ---- options.iou_settings --------------------------------------------------------------------------------------------------------------
def _opt(**ev):
    from shapeclipper_amd.utils.util import EasyDict as edict
    return edict(dict(eval=dict(ev)))


def test_iou_settings():
    from shapeclipper_amd.utils import options
    from shapeclipper_amd.utils.util import EasyDict as edict
    assert options.iou_settings(edict()) is None and options.iou_settings(_opt()) is None          # absent means off
    assert options.iou_settings(_opt(iou=False)) is None
    assert options.iou_settings(_opt(iou_res=64, iou_close=2)) is None                             # settings alone switch nothing on
    assert options.iou_settings(_opt(iou=True)) == (32, 1)
    assert options.iou_settings(_opt(iou=True, iou_res=8, iou_close=0)) == (8, 0)
    assert options.iou_settings(_opt(iou=True, iou_res=64, iou_close=2)) == (64, 2)
    parsed = options.parse_arguments(["--eval.iou", "--eval.iou_res=48", "--eval.iou_close=2"])
    assert options.iou_settings(parsed) == (48, 2)
    assert options.iou_settings(options.parse_arguments(["--eval.iou!"])) is None
    bad = [dict(iou=1), dict(iou="yes"), dict(iou=None), dict(iou_res=7), dict(iou_res=65), dict(iou_res=32.0), dict(iou_res=True),
           dict(iou_res="fine"), dict(iou_res=None), dict(iou_close=-1), dict(iou_close=3), dict(iou_close=1.0), dict(iou_close=True),
           dict(iou_close="yes"), dict(iou_close=None)]
    for on in (False, True):                                    # a bad value raises with the switch off too
        for b in bad:
            with pytest.raises(ValueError):
                options.iou_settings(_opt(**dict(dict(iou=on), **b)))
    assert not [k for k in options.HIP if "iou" in k]           # evaluation settings, not hip.* switches


# ---- the ops: the refusals that need no device -------------------------------------------------------------------------------------------
def test_voxel_ops_refusals():
    from shapeclipper_amd import _lib, ops
    x, o, p = torch.zeros(2, 8, 3), torch.zeros(2, 3), torch.ones(2)
    for res, close in ((7, 1), (65, 1), (32.0, 1), (True, 1), (32, -1), (32, 3), (32, 1.0), (32, False)):
        with pytest.raises(ValueError):
            ops.voxel_frame(x, x, res, close)
        with pytest.raises(ValueError):
            ops.voxel_solid(x, o, p, res, close)
    with pytest.raises(ValueError):
        ops.voxel_frame(x, torch.zeros(3, 8, 3))                # unequal B
    with pytest.raises(ValueError):
        ops.voxel_frame(x, torch.zeros(2, 0, 3))                # an empty cloud
    with pytest.raises(ValueError):
        ops.voxel_frame(torch.zeros(8, 3), torch.zeros(8, 3))
    with pytest.raises(ValueError):
        ops.voxel_solid(x, torch.zeros(2, 4), p)
    with pytest.raises(ValueError):
        ops.voxel_solid(x, o, torch.ones(3))
    with pytest.raises(ValueError):
        ops.voxel_solid(torch.zeros(2, 0, 3), o, p)
    with pytest.raises(TypeError):
        ops.voxel_frame(x.double(), x)
    with pytest.raises(TypeError):
        ops.voxel_solid(x, o.double(), p)
    with pytest.raises(TypeError):
        ops.voxel_solid(x.numpy(), o, p)
    bits = torch.zeros(2, 8, 8, dtype=torch.int64)
    with pytest.raises(TypeError):
        ops.voxel_iou(bits, bits.int())
    with pytest.raises(ValueError):
        ops.voxel_iou(bits, bits[:, :4])
    with pytest.raises(ValueError):
        ops.voxel_iou(bits[0, 0], bits[0, 0])
    for call in (lambda: ops.voxel_frame(x, x), lambda: ops.voxel_solid(x, o, p), lambda: ops.voxel_iou(bits, bits)):
        with pytest.raises(RuntimeError, match="no CPU fallback") as e:                 # host tensors that pass every check above
            call()
        assert str(e.value) == _lib.NO_CPU
    assert ops.VoxelSolid._fields == ("bits", "shell_voxels", "solid_voxels", "sweeps")


def test_header_declares_the_entry_points_and_the_makefile_builds_them_uncontracted():
    import ctypes
    from shapeclipper_amd import _lib, ops
    for name, n_args in (("sc_voxel_frame", 10), ("sc_voxel_solid", 12), ("sc_voxel_iou", 7)):
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == n_args and name in _lib.SYMBOLS
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    mk = open(os.path.join(root, "shapeclipper_amd", "csrc", "Makefile")).read()
    assert "build/voxel_solid.o: EXTRA := -ffp-contract=off" in mk
    hdr = open(_lib.HEADER_PATH).read()
    for name, value in (("MIN_RES", ops.VOXEL_MIN_RES), ("MAX_RES", ops.VOXEL_MAX_RES), ("MAX_CLOSE", ops.VOXEL_MAX_CLOSE)):
        assert "#define SC_VOXEL_%s %d\n" % (name, value) in hdr and getattr(ref, name) == value


# ---- the writers -------------------------------------------------------------------------------------------------------------------------
def test_writers_of_iou_txt_and_iou_cat_txt(tmp_path):
    from shapeclipper_amd.model import runner
    from shapeclipper_amd.utils.util import EasyDict as edict
    var = edict(idx=torch.tensor([4, 7, 9]), category_label=torch.tensor([1, 0, 1]), iou_res=32,
                iou=torch.tensor([0.5, 0.25, float("nan")], dtype=torch.float64), iou_inter=torch.tensor([10, 5, 0], dtype=torch.int32),
                iou_union=torch.tensor([20, 20, 0], dtype=torch.int32), iou_vox_pred=torch.tensor([12, 9, 0], dtype=torch.int32),
                iou_vox_gt=torch.tensor([18, 16, 0], dtype=torch.int32), iou_shell_pred=torch.tensor([11, 9, 0], dtype=torch.int32),
                iou_shell_gt=torch.tensor([13, 8, 0], dtype=torch.int32))
    rec = runner._iou_records(var)
    assert rec.shape == (3, 10) and rec.dtype == torch.float64
    assert runner.iou_line(rec[0], runner.IOU_COLS[0][1]) == "4 32 0.50000000 10 20 12 18 11 13\n"
    for k in runner.IOU_KEYS:
        var[k + "_icp"] = var[k] + 1
    rec = runner._iou_records(var)
    assert rec.shape == (3, 17)
    assert runner.iou_line(rec[1], runner.IOU_COLS[1][1]) == "7 32 1.25000000 6 21 10 17 10 9\n"

    class Data:
        label2cat = {0: "chair", 1: "sofa"}

    class Stub:
        test_data = Data()
    o = edict(output_path=str(tmp_path), data=edict(num_classes=2))
    runner.Runner._write_iou(Stub(), o, rec[:2])
    assert sorted(os.listdir(tmp_path)) == ["iou.txt", "iou_cat.txt", "iou_cat_icp.txt", "iou_icp.txt"]
    assert open(tmp_path / "iou.txt").read() == "4 32 0.50000000 10 20 12 18 11 13\n7 32 0.25000000 5 20 9 16 9 8\n"
    assert open(tmp_path / "iou_icp.txt").read().splitlines()[0] == "4 32 1.50000000 11 21 13 19 12 14"
    assert open(tmp_path / "iou_cat.txt").read() == "IoU    Count Cat\n0.2498     1 chair\n0.4995     1 sofa\n"     # cd_cat.txt's count + 0.001
    for f in os.listdir(tmp_path):
        os.remove(tmp_path / f)
    runner.Runner._write_iou(Stub(), o, rec[:2, :10], per_sample=False)
    assert os.listdir(tmp_path) == ["iou_cat.txt"]
