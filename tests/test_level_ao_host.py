"""The rule of ops.level_ambient_occlusion on the numpy restatement (tests/level_ao_ref.py), without a GPU: convex shapes are fully open,
a longer reach only closes rays, a floor-wall crease rises from the analytic 0.5 at the wall to exactly 1 beyond the reach, two facing
spheres darken each other on the facing side only, a pit's bottom darkens with the reach, the degenerate rows; and the mesh.ao settings.

The crease's margin is the quadrature error of the 64 directions themselves: the |D . n|-weighted open share of a half-space over
1,000 random normals against the exact 0.5 (ref.half_space_error), its maximum 0.0773 (docs/LAB_NOTEBOOK.md)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import level_ao_ref as ref  # noqa: E402

ALL = np.int64(-1)
CENTRE = (8.0, 8.0, 8.0)


def test_the_surface_this_file_tests_exists():
    from shapeclipper_amd import ops
    from shapeclipper_amd.utils import options
    assert hasattr(ops, "level_ambient_occlusion") and hasattr(ops, "ao_directions") and hasattr(options, "MESH_SHADE_TABLE")


def test_directions_are_the_fibonacci_set_and_match_the_product():
    from shapeclipper_amd import ops
    D = ref.directions()
    assert D.shape == (64, 3) and D.dtype == np.float32
    assert np.array_equal(D.view(np.uint32), ops.ao_directions().view(np.uint32))
    assert np.abs(np.linalg.norm(D.astype(np.float64), axis=1) - 1).max() < 1e-7
    assert np.array_equal(D[:, 2], (1 - (2 * np.arange(64.0) + 1) / 64).astype(np.float32))
    assert np.abs(D.astype(np.float64).sum(axis=0)).max() < 0.5            # the set is balanced: no preferred side
    assert ref.step_count(4.0, 0.5) == ops.ao_step_count(4.0, 0.5) == 8 and ops.ao_step_count(4.1, 0.5) == 9
    for radius, step in ((0.0, 0.5), (1.0, 0.0), (4097 * 0.5, 0.5), (float("nan"), 0.5), (1.0, float("inf")), (True, 0.5)):
        with pytest.raises(ValueError, match="level_ambient_occlusion"):
            ops.ao_step_count(radius, step)
    assert ops.ao_step_count(2048.0, 0.5) == 4096


def test_pairwise_tree_is_the_butterflys_order():
    rng = np.random.default_rng(0)
    a = rng.normal(size=(5, 64)).astype(np.float32)
    want = []
    for row in a:
        x = list(row)
        while len(x) > 1:
            x = [np.float32(x[2 * k] + x[2 * k + 1]) for k in range(len(x) // 2)]
        want.append(x[0])
    assert np.array_equal(ref.tree_sum(a), np.array(want, np.float32))


@pytest.mark.parametrize("shape", ["sphere", "box"])
def test_convex_shapes_are_open_everywhere(shape):
    level = ref.sphere_level() if shape == "sphere" else ref.box_level()
    verts = ref.mc_vertices(shape, level)
    normals = (ref.sphere_normals if shape == "sphere" else ref.box_normals)(verts, CENTRE)
    assert len(verts) > 300
    for radius in (2.0, 6.0):
        ao, mask = ref.ambient_occlusion(level[None], verts, normals, np.zeros(len(verts)), radius)
        assert (mask == ALL).all() and (ao == 1).all()


def test_a_longer_reach_only_closes_rays():
    level = ref.two_spheres_level()
    verts = ref.mc_vertices("two_spheres", level)
    c1, c2, _ = ref.TWO_SPHERES
    normals = np.where((verts[:, :1] < 8.5), ref.sphere_normals(verts, c1), ref.sphere_normals(verts, c2))
    masks = [ref.ambient_occlusion(level[None], verts, normals, np.zeros(len(verts)), r)[1] for r in (1.0, 2.5, 6.0)]
    for near, far in zip(masks, masks[1:]):
        assert ((far & ~near) == 0).all()                  # open at the longer reach -> open at the shorter
    assert (ref.popcount(masks[2]) < ref.popcount(masks[0])).any()


def _crease(xs, radius, at=8.0):
    level = ref.crease_level(33, at)
    points = np.array([[x, 16.0, at] for x in xs], np.float32)
    normals = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (len(xs), 1))
    return ref.ambient_occlusion(level[None], points, normals, np.zeros(len(xs)), radius)


def test_crease_rises_from_the_wall_and_is_one_beyond_the_reach():
    xs = np.arange(8.0, 20.5, 0.5)
    radius = 6.0
    ao, mask = _crease(xs, radius)
    print("crease ao:", " ".join("%.4f" % a for a in ao))
    assert (np.diff(ao) >= 0).all() and ao[0] < ao[-1]
    beyond = xs - 8.0 > radius
    assert beyond.sum() >= 5 and (ao[beyond] == 1).all() and (mask[beyond] == ALL).all()
    assert (ao[~beyond][:8] < 1).all()


def test_crease_at_the_wall_is_the_analytic_half_within_the_quadrature_error():
    err = ref.half_space_error(1000, seed=0)
    margin = float(np.abs(err).max())
    print("half-space quadrature error of the 64 directions over 1000 normals: max %.6f mean %.6f" % (margin, float(np.abs(err).mean())))
    assert 0.0 < margin < 0.1        # one direction carries about 1 / 32 of the weight: the error is a few directions' worth
    ao, _ = _crease([8.0], 12.0)                            # on the wall's foot: the rays with d.x < 0 meet the wall at their first sample
    print("crease at the wall:", ao)
    assert abs(float(ao[0]) - 0.5) <= margin


def test_two_facing_spheres_darken_the_facing_side_only():
    level = ref.two_spheres_level()
    verts = ref.mc_vertices("two_spheres", level)
    c1, c2, r = ref.TWO_SPHERES
    first = verts[:, 0] < 8.5
    verts = verts[first]
    normals = ref.sphere_normals(verts, c1)
    ao, mask = ref.ambient_occlusion(level[None], verts, normals, np.zeros(len(verts)), 6.0)
    facing, far = normals[:, 0] > 0.8, normals[:, 0] < -0.5
    assert facing.sum() >= 5 and far.sum() >= 20
    print("two spheres: facing %.4f far %.4f" % (ao[facing].mean(), ao[far].mean()))
    assert (ao[far] == 1).all() and (mask[far] == ALL).all()
    assert (ao[facing] < 1).all() and ao[facing].max() < 0.95


def test_the_bottom_of_a_pit_darkens_with_the_reach():
    level = ref.pit_level()
    p = np.array([[ref.PIT["centre"], ref.PIT["centre"], ref.PIT["bottom"]]], np.float32)
    n = np.array([[0.0, 0.0, 1.0]], np.float32)
    aos = [float(ref.ambient_occlusion(level[None], p, n, [0], r)[0][0]) for r in (1.0, 3.0, 4.5, 7.0)]
    print("pit bottom ao by reach:", aos)
    assert all(b <= a for a, b in zip(aos, aos[1:])) and aos[0] == 1.0 and aos[-1] < aos[1] < 1.0
    # the rays start 4 pitches below the mouth, a square of half-side 2: every ray outside the cone over the mouth's circumscribed circle
    # (tan^2 = 8 / 16) meets a wall within 2.83 / sin(26.6 deg) = 6.4 < 7 pitches, and that cone's cos-weighted share is
    # tan^2 / (1 + tan^2) = 1 / 3; the 64 directions add their half-space quadrature error at the most
    assert aos[-1] <= 1.0 / 3.0 + float(np.abs(ref.half_space_error(1000, seed=0)).max())


def test_degenerate_rows_are_open():
    level = ref.sphere_level()
    nan, inf = float("nan"), float("inf")
    points = np.array([[nan, 8, 8], [8, 8, 2.7], [8, 8, 2.7], [8, 8, 2.7], [40, 8, 8], [-3, -3, -3], [8, inf, 8]], np.float32)
    normals = np.array([[0, 0, -1], [0, 0, 0], [0, nan, -1], [inf, 0, 0], [1, 0, 0], [0, 0, -1], [0, 0, -1]], np.float32)
    ao, mask = ref.ambient_occlusion(level[None], points, normals, np.zeros(len(points)), 4.0)
    assert (ao == 1).all() and (mask == ALL).all()
    # an inward normal at the same place is not degenerate: the rays start inside the solid
    ao, mask = ref.ambient_occlusion(level[None], [[8, 8, 2.7]], [[0, 0, 1]], [0], 4.0)
    assert ao[0] == 0 and mask[0] == 0
    with pytest.raises(ValueError, match="bad_image"):
        ref.ambient_occlusion(level[None], [[8, 8, 2.7]], [[0, 0, -1]], [1], 4.0)


def test_the_empty_cell_rule_is_the_bit_volume():
    """A sample can occlude only in a cell with a corner below iso: skipping the cells the bit volume calls empty changes nothing.  (The
    trilinear value of a cell without such a corner is a convex mix of values >= iso -- up to rounding, which is why it is a rule.)"""
    level = ref.pit_level()
    bits = ref.cell_bits(level[None], 0.0)[0]
    S = level.shape[0]
    assert bits.shape == (S - 1,) * 3 and 0 < bits.sum() < bits.size
    assert not bits[:, :, 9:].any() and bits[:, :, :2].all()               # free space above the floor, solid deep below


def test_settings_table_and_ao_settings(tmp_path):
    from shapeclipper_amd.utils import options
    from shapeclipper_amd.utils.util import EasyDict as edict
    assert [(r.key, r.default, r.kind, r.flag) for r in options.MESH_SHADE_TABLE] == [
        ("ao", False, bool, ""), ("ao_radius", 0.125, (0.0, 1.0), "str")]
    assert list(options.MESH_SHADE) == ["ao", "ao_radius"]
    assert not set(options.MESH_SHADE) & (set(options.MESH) | set(options.MESH_CHECK) | set(options.MESH_DECIMATE))
    assert options.ao_settings(edict()) is None and options.ao_settings(edict(mesh=edict())) is None
    assert options.ao_settings(edict(mesh=edict(ao=False, ao_radius=0.5)), 65) is None
    on = edict(mesh=edict(ao=True))
    assert options.ao_settings(on) == 0.125 and options.ao_settings(on, 65) == 8.0 and options.ao_settings(on, 17) == 2.0
    assert options.ao_settings(edict(mesh=edict(ao=True, ao_radius="2.5e-1")), 33) == 8.0
    assert options.ao_settings(edict(mesh=edict(ao=True, ao_radius=1)), 33) == 32.0
    for bad, what in ((dict(ao=1), "mesh.ao must be a bool"), (dict(ao="yes"), "mesh.ao must be a bool"),
                      (dict(ao_radius=0.0), "mesh.ao_radius must be a float"), (dict(ao_radius=1.5), "mesh.ao_radius must be a float"),
                      (dict(ao=True, ao_radius="wide"), "mesh.ao_radius must be a float"), (dict(ao_radius=True), "mesh.ao_radius must be")):
        with pytest.raises(ValueError, match=what):
            options.ao_settings(edict(mesh=edict(bad)))
    # the command line reaches it, and process_options refuses a bad value with the switch off
    cmd = options.parse_arguments(["--mesh.ao", "--mesh.ao_radius=0.25"])
    assert options.ao_settings(cmd, 17) == 4.0
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    args = ["--yaml=%s/options/pix3d/config.yaml" % root, "--name=pytest_ao", "--output_root=%s" % tmp_path, "--tb!"]
    with pytest.raises(ValueError, match="mesh.ao_radius must be a float"):
        options.set(options.parse_arguments(args + ["--mesh.ao_radius=2"]), verbose=False)
    assert options.ao_settings(options.set(options.parse_arguments(args + ["--mesh.ao"]), verbose=False), 65) == 8.0
    assert options.ao_settings(options.set(options.parse_arguments(args), verbose=False)) is None
