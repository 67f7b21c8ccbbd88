"""The rule of ops.mesh_smooth on the CPU, through its numpy restatement tests/mesh_smooth_ref.py (include/shapeclipper_hip.h,
sc_mesh_smooth), and the mesh.* settings of utils/options.py.  Hand cases with exact answers; the 17^3 marching-cubes shapes of
tests/mesh_simplify_ref.py at the default lam = 0.5, mu = -0.5263 and ten iterations (Taubin keeps the volume within 2 %, plain Laplacian
smoothing loses more than 15 %; a float64 prototype gave 0.75 / 0.67 / 1.32 % against 20.6 / 39.6 / 18.9 % for sphere, torus and cube);
the open rim, duplicate and degenerate faces, an isolated vertex, the face order.  No GPU, no library."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_smooth_ref as ref  # noqa: E402
import mesh_topology_ref as topo  # noqa: E402

SHAPES = ("sphere", "torus", "cube")
_RUN = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _smoothed(name, mu):
    """Ten iterations at lam = 0.5 of a 17^3 shape, computed once: (verts, faces, result)."""
    if (name, mu) not in _RUN:
        verts, faces = ref.shape(name)
        _RUN[(name, mu)] = (verts, faces, ref.mesh_smooth(verts, faces, 10, ref.LAM, mu))
    return _RUN[(name, mu)]


def test_the_default_mu_is_the_pass_band_a_tenth():
    assert ref.MU == -0.5263157894736842 == 1.0 / (0.1 - 1.0 / 0.5)


def test_octahedron_collapses_to_the_origin_in_one_full_laplacian_step():
    out = ref.mesh_smooth(ref.OCTA_V, ref.OCTA_F, 1, lam=1.0, mu=0.0)
    assert out["free"] == 6 and out["fixed_boundary"] == 0 and out["isolated"] == 0 and out["degree_max"] == 4
    assert np.array_equal(out["verts"], np.zeros((6, 3), np.float32))
    assert out["rough_before"] == 1.0 and out["disp_mean"] == 1.0 and out["disp_max"] == 1.0 and out["rough_after"] == 0.0


def test_hexagon_fan_moves_the_hub_half_way_and_keeps_the_rim():
    out = ref.mesh_smooth(ref.HEX_V, ref.HEX_F, 1, lam=0.5, mu=0.0)
    assert out["free"] == 1 and out["fixed_boundary"] == 6 and out["isolated"] == 0 and out["degree_max"] == 6
    assert out["verts"][6].tolist() == [0.0, 0.0, 0.5]
    assert np.array_equal(_bits(out["verts"][:6]), _bits(ref.HEX_V[:6]))
    assert out["fixed_mask"].tolist() == [True] * 6 + [False]
    assert out["rough_before"] == 1.0 and out["rough_after"] == 0.5 and out["disp_mean"] == 0.5 == out["disp_max"]


@pytest.mark.parametrize("name", SHAPES + ("plate", "cut_sphere"))
def test_no_iteration_returns_the_input_bits(name):
    verts, faces = ref.shape(name)
    out = ref.mesh_smooth(verts, faces, 0)
    assert np.array_equal(_bits(out["verts"]), _bits(verts))
    assert out["disp_mean"] == 0.0 == out["disp_max"] and out["rough_after"] == out["rough_before"]


@pytest.mark.parametrize("name", SHAPES)
def test_taubin_keeps_the_volume_and_the_topology(name):
    verts, faces, out = _smoothed(name, ref.MU)
    before, after = topo.mesh_topology(verts, faces), topo.mesh_topology(out["verts"], faces)
    change = abs(after["volume"] - before["volume"]) / before["volume"]
    print("%s: volume %.4f -> %.4f (%+.3f %%), roughness %.4f -> %.4f, displacement mean %.4f max %.4f"
          % (name, before["volume"], after["volume"], 100 * (after["volume"] / before["volume"] - 1), out["rough_before"], out["rough_after"],
             out["disp_mean"], out["disp_max"]))
    assert before["volume"] > 0 and change < 0.02
    assert out["fixed_boundary"] == 0 and out["isolated"] == 0 and out["free"] == len(verts)
    if name == "cube":
        assert out["rough_after"] < out["rough_before"]
    else:
        assert out["rough_after"] < out["rough_before"] / 2
    for key in ("genus", "watertight", "oriented", "manifold", "components", "euler", "edges", "faces", "vertices"):
        assert after[key] == before[key], key
    assert before["watertight"] and before["oriented"] and before["genus"] == {"sphere": 0, "torus": 1, "cube": 0}[name]


@pytest.mark.parametrize("name", SHAPES)
def test_plain_laplacian_smoothing_shrinks(name):
    verts, faces, out = _smoothed(name, 0.0)
    before, after = topo.mesh_topology(verts, faces), topo.mesh_topology(out["verts"], faces)
    loss = 1.0 - after["volume"] / before["volume"]
    print("%s: mu = 0 loses %.2f %% of the volume" % (name, 100 * loss))
    assert loss > 0.15


def test_the_rim_of_a_cut_sphere_is_exactly_the_fixed_set():
    verts, faces = ref.shape("cut_sphere")
    out = ref.mesh_smooth(verts, faces, 10)
    rim = verts[:, 0] == 0.0                                   # the vertices marching cubes put on the grid face x = 0
    stats = topo.mesh_topology(verts, faces)
    assert stats["boundary_edges"] > 0 and rim.sum() == stats["boundary_edges"]       # one closed rim: as many vertices as edges
    assert np.array_equal(out["fixed_mask"], rim)
    assert out["fixed_boundary"] == int(rim.sum()) and out["free"] == len(verts) - int(rim.sum()) and out["isolated"] == 0
    assert np.array_equal(_bits(out["verts"][rim]), _bits(verts[rim]))
    assert (_bits(out["verts"][~rim]) != _bits(verts[~rim])).any(axis=1).mean() > 0.9


def test_duplicate_and_degenerate_faces_change_no_neighbour_set():
    verts, faces = ref.shape("sphere")
    rows, fixed = ref.neighbours(faces, len(verts))
    a, b, c = faces[5].tolist()
    more = np.concatenate([faces, faces[:40], [[a, a, b], [c, b, c], [a, a, a]]]).astype(np.int32)
    rows_more, fixed_more = ref.neighbours(more, len(verts))
    assert rows_more == rows and not fixed.any() and not fixed_more.any()
    want, got = ref.mesh_smooth(verts, faces, 3), ref.mesh_smooth(verts, more, 3)
    assert np.array_equal(_bits(got["verts"]), _bits(want["verts"]))
    # a face with a repeated corner has ONE edge, once: alone it is an edge of count 1
    assert ref.edge_counts([[0, 0, 1]], 2) == {(0, 1): 1} and ref.edge_counts([[2, 2, 2]], 3) == {}


def test_an_isolated_vertex_is_counted_and_kept():
    verts, faces = ref.shape("torus")
    far = np.array([[100.0, -3.0, 0.25]], np.float32)
    out = ref.mesh_smooth(np.concatenate([verts, far]), np.concatenate([faces, [[len(verts)] * 3]]), 4)
    assert out["isolated"] == 1 and out["free"] == len(verts) and out["fixed_boundary"] == 0
    assert np.array_equal(_bits(out["verts"][-1]), _bits(far[0]))
    assert np.array_equal(_bits(out["verts"][:-1]), _bits(ref.mesh_smooth(verts, faces, 4)["verts"]))


def test_the_face_order_changes_no_bit():
    verts, faces = ref.shape("cut_sphere")
    want = ref.mesh_smooth(verts, faces, 5)
    order = np.random.RandomState(4).permutation(len(faces))
    got = ref.mesh_smooth(verts, np.roll(faces[order], 1, axis=1), 5)
    assert np.array_equal(_bits(got["verts"]), _bits(want["verts"]))
    for key in ref.INTS + ref.MEASURES:
        assert got[key] == want[key], key


def test_bad_inputs_are_named():
    with pytest.raises(ValueError, match="bad_vertex"):
        ref.mesh_smooth(np.array([[0, 0, np.nan], [1, 0, 0], [0, 1, 0]], np.float32), [[0, 1, 2]], 1)
    with pytest.raises(ValueError, match="bad_index"):
        ref.mesh_smooth(ref.OCTA_V, [[0, 1, 6]], 1)


# ---- the mesh.* settings -------------------------------------------------------------------------------------------------------------------
def _opt(**mesh):
    from shapeclipper_amd.utils.util import EasyDict as edict
    return edict(mesh=mesh) if mesh else edict()


def test_defaults_and_an_absent_group():
    from shapeclipper_amd.utils import options
    assert [row.key for row in options.MESH_TABLE] == ["smooth", "smooth_lambda", "smooth_band"]
    for opt in (_opt(), _opt(smooth_lambda=0.5)):
        assert options.mesh_setting(opt, "smooth") is None and options.mesh_setting(opt, "smooth_lambda") == 0.5
        assert options.mesh_setting(opt, "smooth_band") == 0.1 and options.smooth_settings(opt) is None
    for row in options.MESH_TABLE:
        assert options.mesh_setting(_opt(**{row.key: row.default}), row.key) == row.default
    opt = _opt(smooth=10)
    assert options.smooth_settings(opt) == (10, 0.5, ref.MU)
    assert dict(opt) == dict(mesh=dict(smooth=10))                                  # nothing is written into the option tree
    assert options.smooth_settings(_opt(smooth=1, smooth_lambda="0.25", smooth_band="1e-1")) == (1, 0.25, 1.0 / (0.1 - 4.0))
    assert options.mesh_setting(_opt(smooth_band="1e-1"), "smooth_band") == 0.1
    assert options.mesh_setting(_opt(smooth=100), "smooth") == 100 and options.mesh_setting(_opt(smooth_lambda=1), "smooth_lambda") == 1.0


@pytest.mark.parametrize("on", (False, True))
@pytest.mark.parametrize("key,value,message", [
    ("smooth", True, "mesh.smooth must be an integer in 1..100, got True"),
    ("smooth", 0, "mesh.smooth must be an integer in 1..100, got 0"),
    ("smooth", 101, "mesh.smooth must be an integer in 1..100, got 101"),
    ("smooth", 2.0, "mesh.smooth must be an integer in 1..100, got 2.0"),
    ("smooth", "3", "mesh.smooth must be an integer in 1..100, got '3'"),
    ("smooth", float("nan"), "mesh.smooth must be an integer in 1..100, got nan"),
    ("smooth_lambda", True, "mesh.smooth_lambda must be a float in (0, 1], got True"),
    ("smooth_lambda", None, "mesh.smooth_lambda must be a float in (0, 1], got None"),
    ("smooth_lambda", 0.0, "mesh.smooth_lambda must be a float in (0, 1], got 0.0"),
    ("smooth_lambda", 1.5, "mesh.smooth_lambda must be a float in (0, 1], got 1.5"),
    ("smooth_lambda", float("nan"), "mesh.smooth_lambda must be a float in (0, 1], got nan"),
    ("smooth_lambda", "half", "mesh.smooth_lambda must be a float in (0, 1], got 'half'"),
    ("smooth_band", False, "mesh.smooth_band must be a float in (0, 0.5], got False"),
    ("smooth_band", None, "mesh.smooth_band must be a float in (0, 0.5], got None"),
    ("smooth_band", 0, "mesh.smooth_band must be a float in (0, 0.5], got 0"),
    ("smooth_band", 0.6, "mesh.smooth_band must be a float in (0, 0.5], got 0.6"),
    ("smooth_band", float("nan"), "mesh.smooth_band must be a float in (0, 0.5], got nan"),
    ("smooth_band", float("inf"), "mesh.smooth_band must be a float in (0, 0.5], got inf"),
])
def test_bad_values_are_refused_with_the_switch_on_or_off(on, key, value, message):
    from shapeclipper_amd.utils import options
    mesh = {key: value}
    if on and key != "smooth":
        mesh["smooth"] = 5
    with pytest.raises(ValueError) as err:
        options.smooth_settings(_opt(**mesh))
    assert str(err.value) == message
    with pytest.raises(ValueError) as err:
        options.mesh_setting(_opt(**mesh), key)
    assert str(err.value) == message


@pytest.mark.parametrize("on", (False, True))
@pytest.mark.parametrize("lam,band", [(1.0, 0.1), (0.95, 0.1), (0.7, 0.5), (0.85, 0.25)])
def test_a_pair_that_amplifies_is_refused(on, lam, band):
    from shapeclipper_amd.utils import options
    mesh = dict(smooth_lambda=lam, smooth_band=band, **(dict(smooth=3) if on else {}))
    with pytest.raises(ValueError, match="mesh.smooth_lambda = .* and mesh.smooth_band = .* give mu = .* <= -1"):
        options.smooth_settings(_opt(**mesh))
    assert options.smooth_settings(_opt(smooth=3, smooth_lambda=0.6, smooth_band=0.5)) == (3, 0.6, 1.0 / (0.5 - 1.0 / 0.6))


def test_the_other_tables_are_untouched_and_the_eval_messages_keep_their_bytes():
    from shapeclipper_amd.utils import eval_reports, options
    from shapeclipper_amd.utils.util import EasyDict as edict
    assert len(options.HIP_TABLE) == 35 and "smooth" not in options.HIP and "smooth" not in options.EVAL
    assert [row.key for row in options.EVAL_TABLE] == [
        "texture", "texture_texels", "mesh_render", "dual_mesh", "dual_reg", "icp", "icp_iters", "icp_scale", "normals", "normals_k",
        "mesh_dist", "emd", "emd_points", "emd_eps", "iou", "iou_res", "iou_close", "mesh_stats", "simplify", "simplify_reg"]
    assert [rep.key for rep in eval_reports.REPORTS][:8] == ["components", "icp", "normals", "mesh_dist", "emd", "iou", "mesh_stats", "simplify"]
    assert not [rep.key for rep in eval_reports.REPORTS if "smooth" in rep.key]
    for eval_, message in ((dict(icp=1), "eval.icp must be a bool, got 1"),
                           (dict(simplify=1), "eval.simplify must be an integer in 2..16, got 1"),
                           (dict(emd_eps="x"), "eval.emd_eps must be a float in (0, 0.25], got 'x'")):
        with pytest.raises(ValueError) as err:
            options.eval_setting(edict(eval=eval_), next(iter(eval_)))
        assert str(err.value) == message
