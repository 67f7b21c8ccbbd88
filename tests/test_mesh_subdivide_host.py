"""The rules of ops.mesh_subdivide and ops.mesh_project_step on the CPU, through their numpy restatement tests/mesh_subdivide_ref.py
(include/shapeclipper_hip.h, sc_mesh_subdivide and sc_mesh_project_step), and the two mesh.subdivide* settings of utils/options.py.  Hand
cases with exact answers (octahedron, tetrahedron, one triangle, an edge with three faces, a doubled face pair); the 17^3 marching-cubes
shapes of tests/mesh_smooth_ref.py at levels 1 and 2 through tests/mesh_topology_ref.py; the open rim of the cut sphere; the face order;
one Newton step on an analytic sphere.  No GPU, no library."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_subdivide_ref as ref  # noqa: E402
import mesh_topology_ref as topo  # noqa: E402

SHAPES = ("sphere", "torus", "cube")
_RUN = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _levels(name, levels):
    """A 17^3 shape after `levels` levels, computed once."""
    if (name, levels) not in _RUN:
        _RUN[(name, levels)] = ref.mesh_subdivide(*ref.shape(name)) if levels == 1 else ref.mesh_subdivide(
            _levels(name, levels - 1)["verts"], _levels(name, levels - 1)["faces"])
    return _RUN[(name, levels)]


def test_octahedron_by_hand():
    out = ref.mesh_subdivide(ref.OCTA_V, ref.OCTA_F)
    assert (len(ref.OCTA_V), len(ref.OCTA_F), 12) == (6, 8, 12)
    assert (out["vertices_out"], len(out["faces"]), out["edges"]) == (18, 32, 12) and len(out["verts"]) == 18
    assert topo.mesh_topology(out["verts"], out["faces"])["edges"] == 48
    assert out["sharp_edges"] == 0 and out["fixed_vertices"] == 0 and out["isolated"] == 0 and out["degree_max"] == 4
    assert not out["fixed"].any()
    # every even vertex: 0.625 x + (0.375 / 4) (its four neighbours, which sum to zero)
    assert np.array_equal(_bits(out["verts"][:6]), _bits(np.float32(0.625) * ref.OCTA_V))
    # the edge (1,0,0)-(0,1,0), opposite (0,0,1) and (0,0,-1): it is face 0's first half-edge, so the first new vertex
    assert out["verts"][6].tolist() == [0.375, 0.375, 0.0]
    assert out["faces"][:4].tolist() == [[0, 6, 8], [2, 7, 6], [4, 8, 7], [6, 7, 8]]


def test_tetrahedron_takes_the_degree_three_branch():
    out = ref.mesh_subdivide(topo.TET_V, topo.TET_F)
    assert (out["vertices_out"], out["edges"], len(out["faces"]), out["degree_max"]) == (10, 6, 16, 3)
    # 0.4375 x_i + 0.1875 (the other three): exact in binary
    want = np.float32(0.4375) * topo.TET_V + np.float32(0.1875) * (topo.TET_V.sum(axis=0)[None] - topo.TET_V)
    assert np.array_equal(_bits(out["verts"][:4]), _bits(want))
    assert out["verts"][0].tolist() == [0.1875, 0.1875, 0.1875] and out["verts"][1].tolist() == [0.4375 + 0.0, 0.1875, 0.1875]
    # an odd vertex: edge (0, 2) of face (0, 2, 1), opposite 1 and 3
    assert out["verts"][4].tolist() == [0.125, 0.375, 0.125]
    stats = topo.mesh_topology(out["verts"], out["faces"])
    assert stats["watertight"] and stats["oriented"] and stats["manifold"] and stats["genus"] == 0


def test_a_single_triangle_is_all_sharp():
    verts = np.array([[0, 0, 0], [2, 0, 0], [0, 4, 6]], np.float32)
    out = ref.mesh_subdivide(verts, [[0, 1, 2]])
    assert (out["vertices_out"], out["edges"], out["sharp_edges"], out["fixed_vertices"]) == (6, 3, 3, 6)
    assert out["fixed"].tolist() == [True] * 6
    assert np.array_equal(_bits(out["verts"][:3]), _bits(verts))
    assert out["verts"][3:].tolist() == [[1, 0, 0], [1, 2, 3], [0, 2, 3]]               # edges 0-1, 1-2, 2-0 in half-edge order
    assert out["faces"].tolist() == [[0, 3, 5], [1, 4, 3], [2, 5, 4], [3, 4, 5]]


def test_an_edge_with_three_faces_is_sharp_and_a_doubled_pair_is_interior():
    # three faces around the edge 0-1: count 3, a midpoint, both ends fixed; the other edges have count 1
    verts = np.array([[0, 0, 0], [0, 0, 2], [1, 0, 1], [-1, 1, 1], [-1, -1, 1]], np.float32)
    fan = ref.mesh_subdivide(verts, [[0, 1, 2], [0, 1, 3], [0, 1, 4]])
    assert ref.edge_table([[0, 1, 2], [0, 1, 3], [0, 1, 4]], 5)[(0, 1)] == [3, 0, 2, 4]
    assert fan["edges"] == 7 and fan["sharp_edges"] == 7 and fan["fixed"].all() and fan["verts"][5].tolist() == [0, 0, 1]
    assert np.array_equal(_bits(fan["verts"][:5]), _bits(verts))
    # the same face twice, the second with the other winding: every edge has count 2 and omin == omax, every vertex degree 2
    tri = np.array([[0, 0, 0], [8, 0, 0], [0, 8, 0]], np.float32)
    pair = ref.mesh_subdivide(tri, [[0, 1, 2], [0, 2, 1]])
    assert ref.edge_table([[0, 1, 2], [0, 2, 1]], 3) == {(0, 1): [2, 0, 2, 2], (1, 2): [2, 1, 0, 0], (0, 2): [2, 2, 1, 1]}
    assert pair["edges"] == 3 and pair["sharp_edges"] == 0 and not pair["fixed"].any() and pair["degree_max"] == 2
    assert pair["verts"][0].tolist() == [1.5, 1.5, 0.0]                                  # 0.625 * 0 + (0.375 / 2) * (8 + 0)
    assert pair["verts"][3].tolist() == [3.0, 2.0, 0.0]                                  # 0.375 * (0 + 8), 0.125 * (8 + 8)
    assert pair["faces"][4:].tolist() == [[0, 5, 3], [2, 4, 5], [1, 3, 4], [5, 4, 3]]


@pytest.mark.parametrize("levels", (1, 2))
@pytest.mark.parametrize("name", SHAPES)
def test_closed_shapes_keep_their_topology(name, levels):
    verts, faces = ref.shape(name)
    before = topo.mesh_topology(verts, faces)
    out = _levels(name, levels)
    after = topo.mesh_topology(out["verts"], out["faces"])
    assert after["faces"] == 4 ** levels * before["faces"] == len(out["faces"])
    previous = before if levels == 1 else topo.mesh_topology(_levels(name, 1)["verts"], _levels(name, 1)["faces"])
    assert out["vertices_out"] == previous["vertices"] + previous["edges"] == after["vertices"] and out["edges"] == previous["edges"]
    assert after["watertight"] and after["oriented"] and after["manifold"]
    assert after["genus"] == before["genus"] == {"sphere": 0, "torus": 1, "cube": 0}[name] and after["components"] == before["components"]
    assert out["sharp_edges"] == 0 and out["fixed_vertices"] == 0 and out["isolated"] == 0 and not out["fixed"].any()
    print("%s level %d: %d faces, %d vertices, volume %.4f -> %.4f" % (name, levels, after["faces"], after["vertices"], before["volume"],
                                                                       after["volume"]))


def test_the_rim_of_a_cut_sphere_is_held():
    verts, faces = ref.shape("cut_sphere")
    before = topo.mesh_topology(verts, faces)
    out = ref.mesh_subdivide(verts, faces)
    after = topo.mesh_topology(out["verts"], out["faces"])
    V = len(verts)
    rim = verts[:, 0] == 0.0
    assert before["boundary_edges"] > 0 and after["boundary_edges"] == 2 * before["boundary_edges"] == 2 * out["sharp_edges"]
    assert np.array_equal(out["fixed"][:V], rim) and np.array_equal(_bits(out["verts"][:V][rim]), _bits(verts[rim]))
    table = ref.edge_table(faces, V)
    ordered = sorted(table.items(), key=lambda kv: kv[1][1])
    sharp = np.array([e[1][0] == 1 for e in ordered])
    assert np.array_equal(out["fixed"][V:], sharp) and int(out["fixed"].sum()) == out["fixed_vertices"] == int(rim.sum()) + int(sharp.sum())
    mid = np.array([(verts[lo].astype(np.float64) + verts[hi].astype(np.float64)) * 0.5 for (lo, hi), _ in ordered], np.float64)
    assert np.array_equal(_bits(out["verts"][V:][sharp]), _bits(mid[sharp].astype(np.float32)))
    assert (out["verts"][V:][sharp][:, 0] == 0.0).all()                                 # the rim stays on the grid face
    assert (_bits(out["verts"][:V][~rim]) != _bits(verts[~rim])).any(axis=1).mean() > 0.9


def test_face_order_and_corner_rotation_change_no_position():
    verts, faces = ref.shape("cut_sphere")
    want = ref.mesh_subdivide(verts, faces)
    order = np.random.RandomState(4).permutation(len(faces))
    got = ref.mesh_subdivide(verts, np.roll(faces[order], 1, axis=1))
    key = lambda out: sorted(map(tuple, _bits(out["verts"]).tolist()))
    assert key(got) == key(want)
    # distinct positions: a position names a vertex, and the faces agree after mapping by position (up to the corner rotation)
    assert len(set(key(want))) == len(want["verts"])
    name = lambda out: [tuple(r) for r in _bits(out["verts"]).tolist()]

    def face_set(out):
        names = name(out)
        faces_ = collections.Counter()
        for a, b, c in out["faces"].tolist():
            tri = (names[a], names[b], names[c])
            faces_[min(tri, tri[1:] + tri[:1], tri[2:] + tri[:2])] += 1
        return faces_
    assert face_set(got) == face_set(want)
    fixed_of = lambda out: sorted(n for n, fx in zip(name(out), out["fixed"].tolist()) if fx)
    assert fixed_of(got) == fixed_of(want)
    for k in ref.INTS:
        assert got[k] == want[k], k


def test_bad_inputs_are_named():
    with pytest.raises(ValueError, match="bad_vertex"):
        ref.mesh_subdivide(np.array([[0, 0, np.inf], [1, 0, 0], [0, 1, 0]], np.float32), [[0, 1, 2]])
    with pytest.raises(ValueError, match="bad_index"):
        ref.mesh_subdivide(ref.OCTA_V, [[0, 1, 6]])
    with pytest.raises(ValueError, match="bad_face"):
        ref.mesh_subdivide(ref.OCTA_V, [[0, 1, 0]])


# ---- the Newton step ----------------------------------------------------------------------------------------------------------------------
def _sphere_field(v, centre, r):
    """f = |x - c| - r and g = (x - c) / |x - c| in float64, both rounded to fp32."""
    d = v.astype(np.float64) - centre
    n = np.sqrt((d * d).sum(axis=1))
    return (n - r).astype(np.float32), (d / n[:, None]).astype(np.float32)


@pytest.mark.parametrize("name", ("sphere", "cut_sphere"))
def test_one_step_puts_the_subdivided_sphere_on_the_analytic_sphere(name):
    """With a unit gradient one step is exact along the radius: | |x| - r | <= 1e-5 r afterwards, about 20 fp32 ulp of r for r in [4, 8)
    grid pitches.  Centre and radius are those of the shape's level grid (mesh_simplify_ref.level, mesh_smooth_ref.cut_sphere_level)."""
    import mesh_simplify_ref
    out = _levels(name, 1) if name == "sphere" else ref.mesh_subdivide(*ref.shape(name))
    centre, r = (np.array([1.3, 7.9, 8.2]) if name == "cut_sphere" else np.array(mesh_simplify_ref.CENTRE)), 5.3
    assert 4.0 <= r < 8.0
    f, g = _sphere_field(out["verts"], centre, r)
    free = ~out["fixed"]
    assert np.abs(f[free]).max() > 1e-3 * r                                             # off the sphere before the step
    got = ref.project_step(out["verts"], f, g, out["fixed"], 1.0, 0.5)
    resid = np.abs(np.sqrt(((got.astype(np.float64) - centre) ** 2).sum(axis=1)) - r)
    print("%s: r = %.1f, max | |x| - r | over %d free vertices %.3g before, %.3g after (bound %.3g)"
          % (name, r, int(free.sum()), np.abs(f[free]).max(), resid[free].max(), 1e-5 * r))
    assert resid[free].max() <= 1e-5 * r
    assert np.array_equal(_bits(got[~free]), _bits(out["verts"][~free]))


def test_the_step_is_clamped_and_keeps_what_it_must():
    f32 = np.float32
    v = np.array([[1, 2, 3]] * 8, f32)
    sdf = np.array([4, 4, np.nan, 1, 1, 1, np.inf, 1e30], f32)
    grad = np.array([[2, 0, 0], [2, 0, 0], [1, 0, 0], [0, 0, 0], [np.inf, 0, 0], [0, 1e-7, 0], [0, 0, 1], [1e-5, 0, 0]], f32)
    fixed = np.array([0, 1, 0, 0, 0, 0, 0, 0], bool)
    got = ref.project_step(v, sdf, grad, fixed, 1.0, 0.75)
    # 0: t = 4 / 4, d = (2, 0, 0), length 2 > 0.75: r = 0.375, d = (0.75, 0, 0)
    assert got[0].tolist() == [0.25, 2.0, 3.0]
    # 1 fixed, 2 NaN value, 3 zero gradient, 4 infinite gradient, 5 g2 = 1e-14 < 1e-12, 6 infinite value, 7 l = 1e35 overflows in fp32
    assert np.array_equal(_bits(got[1:]), _bits(v[1:]))
    # no clamp: scale 3, t = 0.5 / 1, d = 1.5 along y
    got = ref.project_step(v[:1], f32([0.5]), f32([[0, 1, 0]]), [False], 3.0, 2.0)
    assert got[0].tolist() == [1.0, 0.5, 3.0]
    assert ref.project_step(v[:1], f32([0.5]), f32([[0, 1, 0]]), [False], 3.0, 0.0)[0].tolist() == [1.0, 2.0, 3.0]
    assert ref.project_step(np.zeros((0, 3), f32), [], np.zeros((0, 3), f32), [], 1.0, 1.0).shape == (0, 3)


# ---- the mesh.subdivide* settings -----------------------------------------------------------------------------------------------------------
def _opt(**mesh):
    from shapeclipper_amd.utils.util import EasyDict as edict
    return edict(mesh=mesh) if mesh else edict()


def test_defaults_and_an_absent_group():
    from shapeclipper_amd.utils import options
    assert [row.key for row in options.MESH_TABLE] == ["smooth", "smooth_lambda", "smooth_band"]
    assert [row.key for row in options.MESH_SUBDIVIDE_TABLE] == ["subdivide", "subdivide_project"]
    assert list(options.MESH) == ["smooth", "smooth_lambda", "smooth_band", "subdivide", "subdivide_project"]
    for opt in (_opt(), _opt(subdivide_project=2), _opt(smooth=3)):
        assert options.mesh_setting(opt, "subdivide") is None and options.mesh_setting(opt, "subdivide_project") == 2
        assert options.subdivide_settings(opt) is None
    opt = _opt(subdivide=1)
    assert options.subdivide_settings(opt) == (1, 2) and dict(opt) == dict(mesh=dict(subdivide=1))      # nothing is written into the tree
    assert options.subdivide_settings(_opt(subdivide=3, subdivide_project=0)) == (3, 0)
    assert options.subdivide_settings(_opt(subdivide=2, subdivide_project=8)) == (2, 8)
    assert options.smooth_settings(_opt(subdivide=2)) is None and options.smooth_settings(_opt(subdivide=2, smooth=4))[0] == 4


@pytest.mark.parametrize("on", (False, True))
@pytest.mark.parametrize("key,value,message", [
    ("subdivide", True, "mesh.subdivide must be an integer in 1..3, got True"),
    ("subdivide", 0, "mesh.subdivide must be an integer in 1..3, got 0"),
    ("subdivide", 4, "mesh.subdivide must be an integer in 1..3, got 4"),
    ("subdivide", 1.0, "mesh.subdivide must be an integer in 1..3, got 1.0"),
    ("subdivide", "2", "mesh.subdivide must be an integer in 1..3, got '2'"),
    ("subdivide_project", False, "mesh.subdivide_project must be an integer in 0..8, got False"),
    ("subdivide_project", None, "mesh.subdivide_project must be an integer in 0..8, got None"),
    ("subdivide_project", -1, "mesh.subdivide_project must be an integer in 0..8, got -1"),
    ("subdivide_project", 9, "mesh.subdivide_project must be an integer in 0..8, got 9"),
    ("subdivide_project", 2.0, "mesh.subdivide_project must be an integer in 0..8, got 2.0"),
    ("subdivide_project", "2", "mesh.subdivide_project must be an integer in 0..8, got '2'"),
])
def test_bad_values_are_refused_with_the_switch_on_or_off(on, key, value, message):
    from shapeclipper_amd.utils import options
    mesh = {key: value}
    if on and key != "subdivide":
        mesh["subdivide"] = 1
    for ask in (options.subdivide_settings, lambda o: options.mesh_setting(o, key)):
        with pytest.raises(ValueError) as err:
            ask(_opt(**mesh))
        assert str(err.value) == message


def test_process_options_checks_the_two_values():
    import inspect
    from shapeclipper_amd.utils import options
    assert "subdivide_settings" in inspect.getsource(options.process_options)
