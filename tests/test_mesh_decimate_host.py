"""The decimation rule of sc_mesh_decimate_round (include/shapeclipper_hip.h) as tests/mesh_decimate_ref.py restates it, on hand meshes
and the 17^3 marching-cubes shapes, without a GPU: what collapses and what never does, the face budget, the genus, the independent set,
the fixed rim -- and the mesh.decimate* settings.  The topology is judged by tests/mesh_topology_ref.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_decimate_ref as ref  # noqa: E402
import mesh_topology_ref as topo  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _closed(verts, faces, genus=0):
    t = topo.mesh_topology(verts, faces)
    assert t["watertight"] and t["oriented"] and t["manifold"] and t["genus"] == genus and t["euler"] == 2 - 2 * genus, t
    return t


def test_the_tetrahedron_never_collapses():
    """Every edge passes the link condition (the two other vertices) and is refused as the tetrahedron case.  The restatement takes any
    target; the op's lowest is 4, the tetrahedron's own face count."""
    got = ref.decimate(topo.TET_V, topo.TET_F, 2)
    assert got["rounds"] == 1 and got["collapses"] == 0 and got["reached"] == 0 and got["rejected_link"] == 6 and got["rejected_flip"] == 0
    assert np.array_equal(_bits(got["verts"]), _bits(topo.TET_V)) and np.array_equal(got["faces"], topo.TET_F)
    assert got["vertex_map"].tolist() == [0, 1, 2, 3] and not got["fixed"].any()
    at_target = ref.decimate(topo.TET_V, topo.TET_F, 4)
    assert at_target["rounds"] == 0 and at_target["reached"] == 1 and np.array_equal(_bits(at_target["verts"]), _bits(topo.TET_V))
    # beside an octahedron in one image: the octahedron goes down to a tetrahedron, then nothing is left to select
    both = ref.decimate(*ref.tet_and_octa(), 4)
    assert len(both["faces"]) == 8 and both["collapses"] == 2 and both["reached"] == 0
    assert both["vertex_map"][:4].tolist() == [0, 1, 2, 3]
    t = topo.mesh_topology(both["verts"], both["faces"])
    assert t["components"] == 2 and t["watertight"] and t["manifold"] and t["oriented"]


def test_the_octahedron_goes_to_six_and_then_to_four_faces():
    six = ref.decimate(ref.OCTA_V, ref.OCTA_F, 6)
    assert len(six["faces"]) == 6 and len(six["verts"]) == 5 and six["collapses"] == 1 and six["rounds"] == 1 and six["reached"] == 1
    _closed(six["verts"], six["faces"])
    assert sorted(six["vertex_map"].tolist()) == [0, 0, 1, 2, 3, 4]
    four = ref.decimate(six["verts"], six["faces"], 4)
    assert len(four["faces"]) == 4 and len(four["verts"]) == 4 and four["reached"] == 1
    _closed(four["verts"], four["faces"])
    direct = ref.decimate(ref.OCTA_V, ref.OCTA_F, 4)
    assert len(direct["faces"]) == 4 and direct["collapses"] == 2 and direct["reached"] == 1
    _closed(direct["verts"], direct["faces"])
    # an odd budget ends one below: two faces go with every collapse
    assert len(ref.decimate(ref.OCTA_V, ref.OCTA_F, 7)["faces"]) == 6


def test_icosphere_320_to_80():
    verts, faces = ref.icosphere(2)
    assert len(faces) == 320
    history = []
    got = ref.decimate(verts, faces, 80, history=history)
    assert len(got["faces"]) == 80 and got["reached"] == 1 and got["rounds"] == len(history) and got["collapses"] == 120
    for r in history:                                       # a closed genus-0 surface after every round
        used = np.unique(r["faces"])
        edges = {tuple(sorted((int(f[c]), int(f[(c + 1) % 3])))) for f in r["faces"] for c in range(3)}
        assert len(used) - len(edges) + len(r["faces"]) == 2
        assert r["selected"] >= 1 and r["collapsed"] == min(r["selected"], r["collapsed"])
        rings = r["rings"]
        for i in range(len(rings)):                         # no two selected edges share a closed neighbourhood
            for j in range(i + 1, len(rings)):
                assert not (rings[i] & rings[j])
        keys = [k for _, _, k in r["edges_selected"]]
        assert keys == sorted(keys) and r["edges_collapsed"] == r["edges_selected"][:r["collapsed"]]
    _closed(got["verts"], got["faces"])
    radius = np.linalg.norm(got["verts"].astype(np.float64), axis=1)
    print("icosphere 320 -> 80: %d rounds, radius %.4f..%.4f" % (got["rounds"], radius.min(), radius.max()))
    assert 0.95 < radius.min() and radius.max() < 1.15
    assert (got["vertex_map"] >= 0).all() and set(got["vertex_map"].tolist()) == set(range(len(got["verts"])))


def test_the_rim_of_the_cut_sphere_keeps_its_bits_and_its_place_in_fixed():
    verts, faces = ref.shape("cut_sphere")
    table = ref.edge_table(faces, len(verts))
    rim = np.zeros(len(verts), bool)
    for (a, b), e in table.items():
        if e[0] != 2:
            rim[a] = rim[b] = True
    assert rim.sum() > 20
    got = ref.decimate(verts, faces, len(faces) // 4)
    assert len(got["faces"]) in (len(faces) // 4, len(faces) // 4 - 1) and got["reached"] == 1 and got["fixed_vertices"] == int(rim.sum())
    where = got["vertex_map"][rim]
    assert (where >= 0).all() and len(set(where.tolist())) == int(rim.sum())                # none removed, none merged
    assert np.array_equal(_bits(got["verts"][where]), _bits(verts[rim]))
    assert got["fixed"][where].all() and int(got["fixed"].sum()) == int(rim.sum())
    t = topo.mesh_topology(got["verts"], got["faces"])
    assert t["boundary_edges"] == topo.mesh_topology(verts, faces)["boundary_edges"] and t["manifold"] and t["oriented"]


@pytest.mark.parametrize("name,genus", (("sphere", 0), ("torus", 1)))
def test_marching_cubes_shapes_keep_their_genus(name, genus):
    verts, faces = ref.shape(name)
    target = len(faces) // 4
    got = ref.decimate(verts, faces, target)
    assert len(got["faces"]) in (target, target - 1) and got["reached"] == 1
    _closed(got["verts"], got["faces"], genus)


def test_refusals_of_the_restatement():
    with pytest.raises(ValueError, match="bad_vertex"):
        ref.one_round(np.array([[0, 0, np.nan], [1, 0, 0], [0, 1, 0]], np.float32), [[0, 1, 2]], 4)
    with pytest.raises(ValueError, match="bad_index"):
        ref.one_round(ref.OCTA_V, [[0, 1, 6]], 4)
    with pytest.raises(ValueError, match="bad_face"):
        ref.one_round(ref.OCTA_V, [[0, 1, 0]], 4)


# ---- the mesh.decimate* settings ------------------------------------------------------------------------------------------------------------
def _opt(**mesh):
    from shapeclipper_amd.utils.util import EasyDict as edict
    return edict(mesh=mesh) if mesh else edict()


def test_the_table_its_defaults_and_an_absent_group():
    from shapeclipper_amd.utils import options
    assert [(r.key, r.default, r.kind, r.flag) for r in options.MESH_DECIMATE_TABLE] == [
        ("decimate", None, (4, 16777216), "absent"), ("decimate_reg", 1e-3, (0.0, 1.0), "str"), ("decimate_rounds", 1024, (1, 4096), "")]
    assert list(options.MESH_DECIMATE) == ["decimate", "decimate_reg", "decimate_rounds"]
    for opt in (_opt(), _opt(decimate_reg=0.5), _opt(smooth=3), _opt(decimate_rounds=7)):
        assert options.decimate_settings(opt) is None
    opt = _opt(decimate=500)
    assert options.decimate_settings(opt) == (500, 1e-3, 1024) and dict(opt) == dict(mesh=dict(decimate=500))   # nothing is written into the tree
    assert options.decimate_settings(_opt(decimate=4, decimate_reg="1e-2", decimate_rounds=1)) == (4, 0.01, 1)
    assert options.decimate_settings(_opt(decimate=16777216, decimate_reg=1, decimate_rounds=4096)) == (16777216, 1.0, 4096)
    assert options.smooth_settings(_opt(decimate=500)) is None and options.subdivide_settings(_opt(decimate=500)) is None
    assert not options.self_intersect_settings(_opt(decimate=500))


@pytest.mark.parametrize("on", (False, True))
@pytest.mark.parametrize("key,value,message", [
    ("decimate", True, "mesh.decimate must be an integer in 4..16777216, got True"),
    ("decimate", 3, "mesh.decimate must be an integer in 4..16777216, got 3"),
    ("decimate", 16777217, "mesh.decimate must be an integer in 4..16777216, got 16777217"),
    ("decimate", 500.0, "mesh.decimate must be an integer in 4..16777216, got 500.0"),
    ("decimate", "500", "mesh.decimate must be an integer in 4..16777216, got '500'"),
    ("decimate_reg", 0, "mesh.decimate_reg must be a float in (0, 1], got 0"),
    ("decimate_reg", 1.5, "mesh.decimate_reg must be a float in (0, 1], got 1.5"),
    ("decimate_reg", None, "mesh.decimate_reg must be a float in (0, 1], got None"),
    ("decimate_reg", "small", "mesh.decimate_reg must be a float in (0, 1], got 'small'"),
    ("decimate_reg", True, "mesh.decimate_reg must be a float in (0, 1], got True"),
    ("decimate_rounds", 0, "mesh.decimate_rounds must be an integer in 1..4096, got 0"),
    ("decimate_rounds", 4097, "mesh.decimate_rounds must be an integer in 1..4096, got 4097"),
    ("decimate_rounds", None, "mesh.decimate_rounds must be an integer in 1..4096, got None"),
    ("decimate_rounds", 8.0, "mesh.decimate_rounds must be an integer in 1..4096, got 8.0"),
])
def test_bad_values_are_refused_with_the_switch_on_or_off(on, key, value, message):
    from shapeclipper_amd.utils import options
    mesh = {key: value}
    if on and key != "decimate":
        mesh["decimate"] = 500
    with pytest.raises(ValueError) as err:
        options.decimate_settings(_opt(**mesh))
    assert str(err.value) == message


def test_process_options_asks_and_the_pinned_tables_are_unchanged():
    import inspect
    from shapeclipper_amd.utils import eval_reports, options
    assert "decimate_settings" in inspect.getsource(options.process_options)
    assert [row.key for row in options.MESH_TABLE] == ["smooth", "smooth_lambda", "smooth_band"]
    assert [row.key for row in options.MESH_SUBDIVIDE_TABLE] == ["subdivide", "subdivide_project"]
    assert list(options.MESH) == ["smooth", "smooth_lambda", "smooth_band", "subdivide", "subdivide_project"]
    assert [row.key for row in options.MESH_CHECK_TABLE] == ["self_intersect"] and list(options.MESH_CHECK) == ["self_intersect"]
    assert len(options.HIP_TABLE) == 35 and len(options.EVAL_TABLE) == 20
    assert not [k for k in list(options.HIP) + list(options.EVAL) if "decimate" in k]
    assert not [rep.key for rep in eval_reports.REPORTS if "decimate" in rep.key]
    assert [rep.key for rep in eval_reports.REPORTS][:8] == ["components", "icp", "normals", "mesh_dist", "emd", "iou", "mesh_stats", "simplify"]


def test_the_entry_points_are_declared_and_wired():
    from shapeclipper_amd import _lib, ops
    from shapeclipper_amd.utils import eval_3D
    for name in ("sc_mesh_decimate_round", "sc_mesh_decimate_compact"):
        assert name in _lib.SYMBOLS
    assert "sc_mesh_decimate_scratch_bytes" in _lib.SYMBOLS_OTHER
    assert len(_lib.SIGNATURES["sc_mesh_decimate_round"][1]) == 17 and len(_lib.SIGNATURES["sc_mesh_decimate_compact"][1]) == 16
    assert ops.DecimatedMesh._fields == ("verts", "faces", "v_count", "f_count", "vertex_map", "fixed", "rounds", "collapses", "rejected_link",
                                         "rejected_flip", "fixed_vertices", "reached")
    assert eval_3D.INTERSECT_VARIANTS[:5] == ("mc", "dual", "simplified", "smooth", "subdiv") and eval_3D.INTERSECT_VARIANTS[5:] == ("decimated",)
    assert callable(eval_3D.meshes_decimated) and callable(eval_3D.decimated_lines)
