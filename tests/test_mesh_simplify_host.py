"""Properties of the numpy restatement tests/mesh_simplify_ref.py of sc_mesh_cluster_simplify (include/shapeclipper_hip.h) on inputs
checked here, without a GPU: the marching-cubes shapes stay closed manifolds of their genus, the quadric placement recovers the corners
marching cubes chamfers, coincident faces cancel or leave one, the face order decides nothing, and the two option keys refuse bad
values.  tests/test_gpu_mesh_simplify.py holds the kernel to this restatement bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_simplify_ref as ref  # noqa: E402
import mesh_topology_ref as topo  # noqa: E402

SHAPES = ("sphere", "torus", "cube", "plate")


def _simplify(name, pitch, reg=0.05):
    verts, faces = ref.mc_mesh(name)
    return ref.cluster_simplify(verts, faces, (0, 0, 0), pitch, ref.cells_for(pitch), reg)


@pytest.mark.parametrize("name", SHAPES)
def test_marching_cubes_shapes_stay_closed_manifolds_of_their_genus(name):
    verts, faces = ref.mc_mesh(name)
    before = topo.mesh_topology(verts, faces)
    assert before["watertight"] and before["manifold"] and before["oriented"] and before["genus"] == ref.GENUS[name]
    for pitch in (2, 3, 4):
        out = _simplify(name, pitch)
        after = topo.mesh_topology(out["verts_out"], out["faces_out"])
        print("%s pitch %d: faces %d -> %d, vertices %d -> %d, collapsed %d, cancelled %d, genus %d" % (
            name, pitch, len(faces), len(out["faces_out"]), len(verts), len(out["verts_out"]), out["collapsed"], out["cancelled"], after["genus"]))
        assert after["watertight"] and after["manifold"] and after["oriented"] and after["genus"] == ref.GENUS[name], (name, pitch, after)
        assert after["degenerate_faces"] == 0 and len(out["faces_out"]) + out["collapsed"] + out["cancelled"] == len(faces)
        assert np.array_equal(out["faces_out"], out["vertex_cluster"][faces[out["face_source"]]])
        assert (np.diff(out["face_source"]) > 0).all()                      # the output follows the source order
        if pitch == 2:
            assert 3 * len(out["faces_out"]) < len(faces)


def test_prototype_face_counts_of_the_sphere_the_torus_and_the_cube():
    """The counts the rule was prototyped with: the same rule gives the same numbers."""
    assert [len(ref.mc_mesh(n)[1]) for n in ("sphere", "torus", "cube")] == [1088, 1056, 968]
    assert [len(_simplify("sphere", k)["faces_out"]) for k in (2, 3, 4)] == [224, 106, 60]
    assert [len(_simplify("torus", k)["faces_out"]) for k in (2, 3, 4)] == [238, 92, 62]
    assert [len(_simplify("cube", k)["faces_out"]) for k in (2, 3)] == [268, 108]


def test_every_output_vertex_lies_in_its_own_cell():
    for name in SHAPES:
        verts, _ = ref.mc_mesh(name)
        out = _simplify(name, 3)
        for v in range(len(verts)):
            lo = np.floor(verts[v].astype(np.float64) / 3.0)
            new = out["verts_out"][out["vertex_cluster"][v]].astype(np.float64) / 3.0
            assert (new >= lo).all() and (new <= lo + 1).all()


def test_quadric_placement_recovers_the_corners_of_the_cube():
    verts, faces = ref.mc_mesh("cube")
    corners = np.array([[ref.CENTRE[j] + (2 * s[j] - 1) * 4.4 for j in range(3)] for s in np.ndindex(2, 2, 2)])
    worst = lambda p: max(np.sqrt(((p.astype(np.float64) - c) ** 2).sum(axis=1)).min() for c in corners)
    sharp, blunt, mc = worst(_simplify("cube", 3, 0.05)["verts_out"]), worst(_simplify("cube", 3, 1.0)["verts_out"]), worst(verts)
    print("worst corner distance: reg 0.05 %.4f, reg 1 %.4f, marching cubes %.4f" % (sharp, blunt, mc))
    assert sharp < blunt and sharp < mc


def test_a_single_cell_gives_one_vertex_and_no_face():
    verts, faces = ref.mc_mesh("sphere")
    out = ref.cluster_simplify(verts, faces, (0, 0, 0), 16, 1)
    assert out["verts_out"].shape == (1, 3) and out["faces_out"].shape == (0, 3) and out["collapsed"] == len(faces)
    assert (out["vertex_cluster"] == 0).all() and out["cancelled"] == 0
    assert (out["verts_out"] >= 0).all() and (out["verts_out"] <= 16).all()


# four vertices in four cells of a 2-cell box (pitch 1): (0,0,0) (1,0,0) (0,1,0) (0,0,1) cell corners + .25
_V4 = np.array([[.25, .25, .25], [1.25, .25, .25], [.25, 1.25, .25], [.25, .25, 1.25]], np.float32)


def test_two_coincident_opposite_faces_lose_both():
    faces = np.array([[0, 1, 2], [0, 2, 3], [2, 1, 0]], np.int32)
    out = ref.cluster_simplify(_V4, faces, (0, 0, 0), 1, 2)
    assert out["face_source"].tolist() == [1] and out["cancelled"] == 2 and out["collapsed"] == 0
    rotated = np.array([[0, 1, 2], [0, 2, 3], [1, 0, 2]], np.int32)        # the same opposite face, listed from another corner
    assert ref.cluster_simplify(_V4, rotated, (0, 0, 0), 1, 2)["face_source"].tolist() == [1]


def test_two_coincident_like_oriented_faces_keep_the_lower_one():
    faces = np.array([[0, 2, 3], [1, 2, 0], [0, 1, 2], [2, 0, 1]], np.int32)
    out = ref.cluster_simplify(_V4, faces, (0, 0, 0), 1, 2)
    assert out["face_source"].tolist() == [0, 1] and out["cancelled"] == 2
    assert out["faces_out"].tolist() == out["vertex_cluster"][faces[[0, 1]]].tolist()      # the kept face keeps its rotation
    three = np.array([[0, 1, 2], [2, 1, 0], [1, 2, 0]], np.int32)          # two against one: the lower of the two stays
    assert ref.cluster_simplify(_V4, three, (0, 0, 0), 1, 2)["face_source"].tolist() == [0]


def test_the_face_order_changes_no_vertex_bit_and_no_output_face():
    verts, faces = ref.mc_mesh("torus")
    first = ref.cluster_simplify(verts, faces, (0, 0, 0), 3, 6)
    perm = np.random.RandomState(5).permutation(len(faces))
    again = ref.cluster_simplify(verts, faces[perm], (0, 0, 0), 3, 6)
    assert np.array_equal(first["acc"], again["acc"])
    assert np.array_equal(first["verts_out"].view(np.uint32), again["verts_out"].view(np.uint32))
    assert np.array_equal(first["vertex_cluster"], again["vertex_cluster"])
    as_set = lambda f: sorted(tuple(np.roll(t, -int(np.argmin(t)))) for t in f.tolist())
    assert as_set(first["faces_out"]) == as_set(again["faces_out"])
    assert (first["collapsed"], first["cancelled"]) == (again["collapsed"], again["cancelled"])


def test_bad_vertices_and_indices_are_refused():
    verts, faces = ref.mc_mesh("sphere")
    for value in (np.nan, np.inf, -0.5, 16.5):
        bad = verts.copy()
        bad[7, 1] = value
        with pytest.raises(ValueError, match="bad_vertex"):
            ref.cluster_simplify(bad, faces, (0, 0, 0), 2, 8)
    on_the_face = verts.copy()
    on_the_face[7] = 16.0                                                   # exactly on the upper face: the last cell
    out = ref.cluster_simplify(on_the_face, faces, (0, 0, 0), 2, 8)
    assert out["vertex_cluster"][7] == len(out["verts_out"]) - 1
    bad = faces.copy()
    bad[3, 2] = len(verts)
    with pytest.raises(ValueError, match="bad_index"):
        ref.cluster_simplify(verts, bad, (0, 0, 0), 2, 8)


def test_options_refuse_every_bad_value_of_the_two_keys():
    from shapeclipper_amd.utils import options
    from shapeclipper_amd.utils.util import EasyDict as edict
    assert options.simplify_settings(edict()) is None and options.simplify_settings(edict(eval=dict(vox_res=64))) is None
    assert options.simplify_settings(edict(eval=dict(simplify=2))) == (2, 0.05)
    assert options.simplify_settings(edict(eval=dict(simplify=16, simplify_reg=1))) == (16, 1.0)
    assert options.simplify_settings(edict(eval=dict(simplify=4, simplify_reg="1e-3"))) == (4, 1e-3)
    assert options.simplify_settings(edict(eval=dict(simplify_reg=0.5))) is None
    for k in (True, False, 1, 17, 0, -2, 2.0, "2x", [2]):
        with pytest.raises(ValueError, match="eval.simplify "):
            options.simplify_settings(edict(eval=dict(simplify=k)))
    for reg in (True, 0, 0.0, -0.1, 1.5, float("nan"), float("inf"), "much", None):
        for on in (dict(simplify=2), dict()):                               # whether or not the switch is on
            with pytest.raises(ValueError, match="eval.simplify_reg"):
                options.simplify_settings(edict(eval=dict(on, simplify_reg=reg)))
    assert options.parse_arguments(["--eval.simplify=3"]).eval.simplify == 3
