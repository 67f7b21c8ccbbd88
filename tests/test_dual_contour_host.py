"""Dual contouring without a GPU: the numpy restatement (tests/dual_contour_ref.py) on a hand-worked cell and against float64, and the
`--eval.dual_mesh` / `--eval.dual_reg` options."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dual_contour_ref as R  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_hand_worked_corner_cell():
    """One inside corner, (3,3,3) of cell (2,2,2): crossings (2.5,3,3), (3,2.5,3), (3,3,2.5) with axis normals.  c = 17/6 each,
    sum n n^T = I, reg k = 0.15, b_j = -1/3: every coordinate is 17/6 - (1/3) / 1.15."""
    want = 17.0 / 6.0 - (1.0 / 3.0) / 1.15
    P = [np.array(p, np.float32) for p in ((2.5, 3, 3), (3, 2.5, 3), (3, 3, 2.5))]
    for sign in (1.0, -1.0):                                    # n n^T and n (n . d) are even in n
        N = [sign * np.eye(3, dtype=np.float32)[j] for j in range(3)]
        x = R.solve_cell_fp32((2, 2, 2), P, N, 0.05)
        assert all(type(v) is np.float32 for v in x)
        assert np.abs(np.array(x, np.float64) - want).max() <= 4 * np.spacing(np.float32(want))
        assert np.abs(np.array(R.solve_cell_exact((2, 2, 2), P, N, 0.05)) - want).max() <= 1e-14
    # the same cell through the whole mesher: a single inside grid point has 6 crossings, 8 cells around it and one quad per crossing
    level = np.ones((6, 6, 6), np.float32)
    level[3, 3, 3] = -1.0
    pv, vmap = R.crossings(level)
    assert pv[vmap[(2, 3, 3, 0)]].tolist() == [2.5, 3, 3] and len(pv) == 6
    normals = np.zeros_like(pv)
    for (x, y, z, axis), v in vmap.items():
        normals[v, axis] = 1.0 if (x, y, z) == (3, 3, 3) else -1.0
    verts, faces = R.dual_contour(level, normals, 0.0, 0.05)
    assert verts.shape == (8, 3) and faces.shape == (12, 3)
    assert np.abs(verts[0].astype(np.float64) - want).max() <= 4 * np.spacing(np.float32(want))
    assert np.abs(np.abs(verts.astype(np.float64) - 3.0) - (3.0 - want)).max() <= 1e-6       # the eight vertices mirror each other


def test_fp32_restatement_against_float64():
    """Every grid of the GPU tests: the fp32 restatement stays within 8 times the difference measured on the CPU (dual_contour_ref's
    docstring) of the float64 solve of the same system; the faces do not depend on the arithmetic."""
    worst = 0.0
    for name, (level, normals) in R.grids().items():
        v32, f32_ = R.dual_contour(level, normals, 0.0, 0.05)
        v64, f64 = R.dual_contour(level, normals, 0.0, 0.05, exact=True)
        assert np.array_equal(f32_, f64) and v32.shape == v64.shape
        assert np.isfinite(v32).all() and np.isfinite(v64).all()        # the clamp leaves no NaN, whatever the inputs hold
        diff = float(np.abs(v32.astype(np.float64) - v64).max()) if len(v32) else 0.0
        print("%-8s S=%2d cells=%4d faces=%4d  max |fp32 - float64| = %.9g" % (name, level.shape[0], len(v32), len(f32_), diff))
        worst = max(worst, diff)
    print("worst %.9g, allowed %.9g" % (worst, R.FP32_VS_EXACT_BOUND))
    assert worst <= R.FP32_VS_EXACT_BOUND


def test_every_vertex_lies_in_its_cell_and_faces_are_interior_edges():
    for name, (level, normals) in R.grids().items():
        verts, faces = R.dual_contour(level, normals)
        S = level.shape[0]
        inside = level < 0
        cells = [(x, y, z) for x in range(S - 1) for y in range(S - 1) for z in range(S - 1)
                 if 0 < inside[x:x + 2, y:y + 2, z:z + 2].sum() < 8]
        assert len(cells) == len(verts)
        lo = np.array(cells, np.float32).reshape(-1, 3)
        assert ((verts >= lo) & (verts <= lo + 1)).all(), name
        n_edges = 0
        for a in range(3):
            sl = [slice(1, S - 1)] * 3
            lo_, hi_ = list(sl), list(sl)
            lo_[a], hi_[a] = slice(0, S - 1), slice(1, S)
            n_edges += int((inside[tuple(lo_)] != inside[tuple(hi_)]).sum())
        assert len(faces) == 2 * n_edges, name


def _parse(tmp_path, *extra):
    from shapeclipper_amd.utils import options
    args = ["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_dual_opts", "--output_root=%s" % tmp_path, "--tb!"] + list(extra)
    return options.set(options.parse_arguments(args), verbose=False)


def test_option_parsing(tmp_path):
    from shapeclipper_amd.utils import options
    table = tuple(options.HIP_TABLE)
    off = _parse(tmp_path)
    assert "dual_mesh" not in off.eval and options.dual_mesh_reg(off) is None          # absent means off
    on = _parse(tmp_path, "--eval.dual_mesh")
    assert on.eval.dual_mesh is True and options.dual_mesh_reg(on) == 0.05
    assert options.dual_mesh_reg(_parse(tmp_path, "--eval.dual_mesh", "--eval.dual_reg=0.2")) == 0.2
    assert options.dual_mesh_reg(_parse(tmp_path, "--eval.dual_mesh", "--eval.dual_reg=1.0")) == 1.0
    assert options.dual_mesh_reg(_parse(tmp_path, "--eval.dual_mesh!", "--eval.dual_reg=0.2")) is None
    for bad in ("0", "0.0", "-0.05", "1.5", "abc", "true", ".nan", "[0.1]"):
        with pytest.raises(ValueError, match="eval.dual_reg"):
            _parse(tmp_path, "--eval.dual_mesh", "--eval.dual_reg=%s" % bad)
        with pytest.raises(ValueError, match="eval.dual_reg"):                            # a bad value is refused with the dump off too
            _parse(tmp_path, "--eval.dual_reg=%s" % bad)
    # an evaluation setting beside eval.vox_res: the hip.* table is untouched
    assert tuple(options.HIP_TABLE) == table and len(options.HIP_TABLE) == 35
    assert not any("dual" in row.key for row in options.HIP_TABLE) and "dual_mesh" not in on.hip and "dual_reg" not in on.hip
    assert options.dual_mesh_reg(options.edict()) is None                                # a tree built by hand without an `eval` node


def test_ops_refuses_bad_arguments_before_any_launch():
    """No GPU here: the refusals that come before the library is touched."""
    import torch
    from shapeclipper_amd import ops
    level = torch.zeros(1, 4, 4, 4)
    for reg in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="reg"):
            ops.dual_contour_mesh(level, torch.zeros(0, 3), 0.0, reg)
    for normals in (torch.zeros(5), torch.zeros(5, 2), torch.zeros(5, 3, dtype=torch.float64), None):
        with pytest.raises(ValueError, match="normals"):
            ops.dual_contour_mesh(level, normals)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                            # isosurface_mesh's refusal of host tensors
        ops.dual_contour_mesh(level, torch.zeros(0, 3))
