"""The self-intersection rule of sc_mesh_self_intersections without a GPU: the numpy restatement (tests/mesh_intersect_ref.py) against
the same predicate in exact rational arithmetic on three triangle soups, on hand cases, on the 17^3 marching-cubes shapes and what the
post-processing steps make of them, under a permutation of the faces; and the `--mesh.self_intersect` setting."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import mesh_intersect_ref as ref        # noqa: E402
import mesh_simplify_ref                # noqa: E402
import mesh_smooth_ref                  # noqa: E402
import mesh_subdivide_ref               # noqa: E402

SHAPES = ("sphere", "torus", "cube", "plate")


@pytest.fixture(autouse=True)
def _the_feature_exists():
    """The restatement describes ops.mesh_self_intersections and its setting; the header states the rule it restates."""
    from shapeclipper_amd import ops
    from shapeclipper_amd.utils import options
    assert hasattr(ops, "mesh_self_intersections") and hasattr(options, "MESH_CHECK_TABLE")
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "shapeclipper_hip.h")).read()
    assert "int sc_mesh_self_intersections(" in header and "2^-49" in header


# ---- against exact arithmetic ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "lattice", "half"])
def test_the_restatement_has_no_false_hit_and_no_miss_against_exact_arithmetic(kind):
    verts, faces = ref.soup(kind)
    assert verts.shape == (40, 3) and faces.shape == (60, 3) and not ref.degenerate(faces).any()
    A, B = np.triu_indices(60, k=1)
    assert len(A) == 1770                                               # every pair, none skipped
    shared, hit = ref.pair_hits(verts, faces, A, B)
    exact = [ref.exact_pair(verts, faces[a].tolist(), faces[b].tolist()) for a, b in zip(A.tolist(), B.tolist())]
    exact_hit = np.asarray([e[0] for e in exact])
    decided = np.asarray([e[1] for e in exact])
    print("%s: %d hits, %d exact hits, %d pairs with a zero exact sign, %d share two or more" % (
        kind, int(hit.sum()), int(exact_hit.sum()), int((~decided).sum()), int((shared >= 2).sum())))
    assert not (hit & ~exact_hit).any()                                 # no false hit
    assert not (exact_hit & decided & ~hit).any()                       # no miss among the pairs whose exact signs are all non-zero
    assert hit.sum() > 100
    # the op's path -- candidates by box overlap only -- counts the same hits: a hit implies that the boxes overlap
    full = ref.image_self_intersections(verts, faces)
    assert full["pairs"] == int(hit.sum()) and int(full["hits"].sum()) == 2 * full["pairs"]
    assert {tuple(p) for p in full["hit_pairs"].tolist()} == {(a, b) for a, b, h in zip(A.tolist(), B.tolist(), hit.tolist()) if h}
    assert full["pairs_vertex"] == int((hit & (shared == 1)).sum())


def test_a_non_zero_sign_is_the_exact_sign():
    rng = np.random.default_rng(5)
    pts = (rng.integers(0, 4, (400, 4, 3)) * 0.5).astype(np.float32)
    pts[::3] += rng.uniform(-1e-6, 1e-6, (134, 4, 3)).astype(np.float32)
    s = ref.sign3(pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3])
    exact = np.asarray([ref.exact_sign3(*p) for p in pts])
    assert (s[s != 0] == exact[s != 0]).all() and (s != 0).sum() > 200 and (s == 0).sum() > 10
    assert (exact[s == 0] == 0).sum() > 10


# ---- hand cases ---------------------------------------------------------------------------------------------------------------------------
HAND, _case = ref.HAND, ref.hand_case


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(name):
    verts, faces = _case(name)
    r = ref.image_self_intersections(np.asarray(verts, np.float32), np.asarray(faces, np.int32))
    pairs, pairs_vertex, deg = HAND[name]
    assert (r["pairs"], r["pairs_vertex"], r["degenerate"]) == (pairs, pairs_vertex, deg)
    assert r["faces_hit"] == 2 * pairs and int(r["hits"].sum()) == 2 * pairs
    if pairs:
        assert r["partner"].tolist() == [1, 0] and r["box_pairs"] == 1
    else:
        assert (r["partner"] == -1).all()
    if name == "duplicate":
        assert r["box_pairs"] == 0              # three shared indices: not a pair at all
    if name == "degenerate":
        assert r["box_pairs"] == 0 and r["hits"].tolist() == [0, 0]
    if name != "degenerate":                    # the exact predicate agrees
        f = np.asarray(faces)
        exact = [ref.exact_pair(np.asarray(verts, np.float32), f[a].tolist(), f[b].tolist())[0] for a in range(len(f)) for b in range(a + 1, len(f))]
        assert sum(exact) == pairs


def test_flags():
    verts, faces = _case("crossing")
    bad = np.asarray(verts, np.float32)
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="bad_vertex"):
        ref.image_self_intersections(bad, faces)
    bad[3, 1] = 1e15
    with pytest.raises(ValueError, match="bad_vertex"):
        ref.image_self_intersections(bad, faces)
    with pytest.raises(ValueError, match="bad_index"):
        ref.image_self_intersections(verts, [[0, 1, 2], [3, 4, 6]])


# ---- the project's own meshes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_the_marching_cubes_shapes_and_their_post_processed_forms_do_not_cross(name):
    verts, faces = mesh_simplify_ref.mc_mesh(name)
    variants = {"mc": (verts, faces)}
    variants["smooth"] = (mesh_smooth_ref.mesh_smooth(verts, faces, 10)["verts"], faces)
    for k in (2, 3, 4):
        s = mesh_simplify_ref.cluster_simplify(verts, faces, (0.0, 0.0, 0.0), float(k), mesh_simplify_ref.cells_for(k))
        variants["simplified%d" % k] = (s["verts_out"], s["faces_out"])
    sub = mesh_subdivide_ref.mesh_subdivide(verts, faces)
    variants["subdiv"] = (sub["verts"], sub["faces"])
    for key, (v, f) in variants.items():
        r = ref.image_self_intersections(v, f)
        print("%s %s: %d faces, %d box pairs, %d pairs" % (name, key, len(f), r["box_pairs"], r["pairs"]))
        assert r["pairs"] == 0 and r["pairs_vertex"] == 0 and r["faces_hit"] == 0 and not r["hits"].any() and (r["partner"] == -1).all()
        assert r["degenerate"] == 0
        A, B = ref.box_pairs(v, f)
        shared, _ = ref.pair_hits(v, f, A, B)
        assert r["box_pairs"] == int((shared <= 1).sum()) > 0


def test_two_spheres_cross_each_other_only():
    verts, faces = ref.two_spheres()
    half = len(faces) // 2
    r = ref.image_self_intersections(verts, faces)
    print("two spheres: %d faces, %d box pairs, %d pairs on %d faces, %d share a vertex" % (
        len(faces), r["box_pairs"], r["pairs"], r["faces_hit"], r["pairs_vertex"]))
    assert r["pairs"] > 0 and int(r["hits"].sum()) == 2 * r["pairs"] and r["pairs_vertex"] == 0
    assert ((r["hit_pairs"][:, 0] < half) & (r["hit_pairs"][:, 1] >= half)).all()          # every hit pair joins the two copies
    hit = r["hits"] > 0
    assert ((r["partner"][hit] >= half) == (np.flatnonzero(hit) < half)).all() and (r["partner"][~hit] == -1).all()


def test_permuting_the_faces_permutes_the_integers():
    verts, faces = ref.two_spheres()
    r = ref.image_self_intersections(verts, faces)
    perm = np.random.default_rng(3).permutation(len(faces))             # new face j is old face perm[j]
    new_of_old = np.argsort(perm)
    p = ref.image_self_intersections(verts, faces[perm])
    for k in ("pairs", "pairs_vertex", "box_pairs", "faces_hit", "degenerate"):
        assert p[k] == r[k]
    assert np.array_equal(p["hits"], r["hits"][perm])
    # partner is the LOWEST face crossed, so it maps through the permutation as a set: the lowest new number among the old partners
    old_pairs = r["hit_pairs"]
    expect = np.full(len(faces), np.iinfo(np.int64).max)
    for a, b in old_pairs.tolist():
        na, nb = new_of_old[a], new_of_old[b]
        expect[na], expect[nb] = min(expect[na], nb), min(expect[nb], na)
    expect[expect == np.iinfo(np.int64).max] = -1
    assert np.array_equal(p["partner"], expect)


def test_a_batch_is_its_images():
    soup = ref.soup("half")
    spheres = ref.two_spheres()
    packed = ref.pack([soup, (np.zeros((0, 3)), np.zeros((0, 3))), spheres])
    out = ref.self_intersections(*packed)
    a, c = ref.image_self_intersections(*soup), ref.image_self_intersections(*spheres)
    assert out["pairs"].tolist() == [a["pairs"], 0, c["pairs"]] and out["box_pairs"].tolist() == [a["box_pairs"], 0, c["box_pairs"]]
    assert out["hits"].dtype == np.int32 and out["partner"].dtype == np.int32 and out["pairs"].dtype == np.int64
    assert np.array_equal(out["partner"], np.concatenate([a["partner"], c["partner"]]))


# ---- the setting --------------------------------------------------------------------------------------------------------------------------
def _opt(**mesh):
    from shapeclipper_amd.utils.util import EasyDict as edict
    return edict(mesh=edict(mesh))


def test_the_setting_defaults_and_bad_values():
    from shapeclipper_amd.utils import options
    from shapeclipper_amd.utils.util import EasyDict as edict
    assert [row.key for row in options.MESH_CHECK_TABLE] == ["self_intersect"]
    assert list(options.MESH_CHECK) == ["self_intersect"] and options.MESH_CHECK["self_intersect"].default is False
    assert options.MESH_CHECK["self_intersect"].kind is bool
    assert options.self_intersect_settings(edict()) is False                        # no `mesh` group at all
    assert options.self_intersect_settings(edict(mesh=None)) is False
    assert options.self_intersect_settings(_opt()) is False
    assert options.self_intersect_settings(_opt(smooth=3)) is False
    assert options.self_intersect_settings(_opt(self_intersect=True)) is True
    assert options.self_intersect_settings(_opt(self_intersect=False)) is False
    for bad in (1, 0, "true", None, 1.0, [True]):
        with pytest.raises(ValueError) as e:
            options.self_intersect_settings(_opt(self_intersect=bad))
        assert str(e.value) == "mesh.self_intersect must be a bool, got %r" % (bad,)


def test_the_command_line_spells_the_switch_and_process_options_checks_it(tmp_path):
    from shapeclipper_amd.utils import options
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    base = ["--yaml=%s/options/pix3d/config.yaml" % root, "--name=pytest_selfx_host", "--output_root=%s" % tmp_path]
    on = options.set(options.parse_arguments(base + ["--mesh.self_intersect"]), verbose=False)
    assert options.self_intersect_settings(on) is True
    off = options.set(options.parse_arguments(base + ["--mesh.self_intersect!"]), verbose=False)
    assert options.self_intersect_settings(off) is False
    absent = options.set(options.parse_arguments(base), verbose=False)
    assert options.self_intersect_settings(absent) is False and "self_intersect" not in (absent.get("mesh", None) or {})
    with pytest.raises(ValueError, match="mesh.self_intersect must be a bool, got 2"):      # checked whether or not anything is on
        options.set(options.parse_arguments(base + ["--mesh.self_intersect=2"]), verbose=False)


def test_the_pinned_tables_are_unchanged():
    from shapeclipper_amd.utils import options
    assert [row.key for row in options.MESH_TABLE] == ["smooth", "smooth_lambda", "smooth_band"]
    assert [row.key for row in options.MESH_SUBDIVIDE_TABLE] == ["subdivide", "subdivide_project"]
    assert list(options.MESH) == ["smooth", "smooth_lambda", "smooth_band", "subdivide", "subdivide_project"]
    assert [row.key for row in options.EVAL_TABLE] == [
        "texture", "texture_texels", "mesh_render", "dual_mesh", "dual_reg", "icp", "icp_iters", "icp_scale", "normals", "normals_k",
        "mesh_dist", "emd", "emd_points", "emd_eps", "iou", "iou_res", "iou_close", "mesh_stats", "simplify", "simplify_reg"]
    assert "self_intersect" not in options.EVAL and "self_intersect" not in options.MESH
