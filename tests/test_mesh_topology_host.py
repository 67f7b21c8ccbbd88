"""Host checks of the mesh statistics (`--eval.mesh_stats`): the numpy restatement tests/mesh_topology_ref.py of sc_mesh_topology's rules
against hand-counted meshes and against scipy's connected components, the settings, and the line format of mesh_stats.txt.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_topology_ref as ref  # noqa: E402

from shapeclipper_amd import ops  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MESHES = ref.meshes()
# the restatement is of THIS op: it names the fields as ops.mesh_topology returns them
assert ref.INT_FIELDS == ops.MESH_TOPOLOGY_COUNTS and ref.FLAGS == ops.MESH_TOPOLOGY_FLAGS


def test_restatement_header_and_op_agree_on_the_constants():
    import re
    header = open(os.path.join(ROOT, "include", "shapeclipper_hip.h")).read()
    assert int(re.search(r"#define SC_MESH_TOPOLOGY_CHUNK (\d+)", header).group(1)) == ref.CHUNK
    assert int(re.search(r"#define SC_MESH_TOPOLOGY_FIELDS (\d+)", header).group(1)) == len(ref.INT_FIELDS) + len(ref.FLAGS)
    assert ops.MeshTopology._fields == ref.INT_FIELDS + ref.FLAGS + ("area", "volume", "face_component")
    assert [ops.mesh_topology_slots(f) for f in (0, 1, 5, 200, 1 << 20)] == [2, 8, 32, 2048, 1 << 23]
    for f in (1, 3, 170, 171, 12345):
        assert ops.mesh_topology_slots(f) >= 6 * f and ops.mesh_topology_slots(f) // 2 < 6 * f + 2


@pytest.mark.parametrize("name", list(MESHES))
def test_restatement_gives_the_hand_counted_numbers(name):
    verts, faces, expected = MESHES[name]
    got = ref.mesh_topology(verts, faces)
    for key, value in expected.items():
        assert got[key] == value, (name, key, got[key], value)
    assert got["euler"] == got["vertices"] - got["edges"] + got["faces"]
    assert got["face_component"].dtype == np.int32 and len(got["face_component"]) == len(faces)


def test_unit_corner_tetrahedron_has_volume_one_sixth_and_the_known_area():
    got = ref.mesh_topology(ref.TET_V, ref.TET_F)
    assert got["volume"] == np.float64(1.0) / np.float64(6.0)
    assert abs(got["area"] - (1.5 + np.sqrt(3.0) / 2)) <= 1e-15
    cube = ref.mesh_topology(ref.CUBE_V, ref.CUBE_F)
    assert abs(cube["volume"] - 1.0) <= 2e-16 * 12 and cube["area"] == 6.0      # oriented outward; twelve terms of n / 6, half an ulp each
    assert ref.mesh_topology(ref.TET_V, ref.TET_F[:, ::-1])["volume"] == -got["volume"]


def test_degenerate_face_and_extra_vertex_change_nothing_else():
    verts, faces, _ = MESHES["tet_degenerate"]
    got, tet = ref.mesh_topology(verts, faces), ref.mesh_topology(ref.TET_V, ref.TET_F)
    for key in ref.INT_FIELDS + ref.FLAGS + ("area", "volume"):
        if key not in ("degenerate_faces", "unreferenced_vertices"):
            assert got[key] == tet[key], key
    assert got["face_component"].tolist() == [0, 0, 0, 0, -1]


def test_components_equal_scipy_on_a_random_soup():
    import scipy.sparse
    from scipy.sparse.csgraph import connected_components
    verts, faces = ref.soup()
    got = ref.mesh_topology(verts, faces)
    live = [f for f in range(len(faces)) if len(set(faces[f].tolist())) == 3]
    assert 0 < got["degenerate_faces"] == len(faces) - len(live)
    edge_sets = [{frozenset((int(faces[f, k]), int(faces[f, (k + 1) % 3]))) for k in range(3)} for f in live]
    rows, cols = zip(*[(i, j) for i in range(len(live)) for j in range(len(live)) if edge_sets[i] & edge_sets[j]])
    graph = scipy.sparse.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(len(live),) * 2)
    n, label = connected_components(graph, directed=False)
    assert got["components"] == n
    lowest = {}                                         # scipy's label -> the lowest face of the class
    for i, f in enumerate(live):
        lowest.setdefault(label[i], f)
    assert got["face_component"][live].tolist() == [lowest[label[i]] for i in range(len(live))]
    assert got["largest_component_faces"] == np.bincount(label).max()
    assert got["nonmanifold_edges"] > 0 and got["genus"] == -1


def test_summation_order_is_by_chunks_of_256_faces():
    """600 faces: three chunks.  The restated sum equals the chunked sum spelled out here and is not the plain running sum's business."""
    rng = np.random.RandomState(5)
    verts = rng.uniform(-1, 1, (50, 3)).astype(np.float32)
    faces = np.stack([rng.permutation(50)[:3] for _ in range(600)]).astype(np.int32)
    got = ref.mesh_topology(verts, faces)
    p = verts.astype(np.float64)
    terms = [ref.face_terms(p[a], p[b], p[c]) for a, b, c in faces]
    total = [np.float64(0.0), np.float64(0.0)]
    for first in (0, 256, 512):
        part = [np.float64(0.0), np.float64(0.0)]
        for t in terms[first:first + 256]:
            part = [part[0] + t[0], part[1] + t[1]]
        total = [total[0] + part[0], total[1] + part[1]]
    assert got["area"] == total[0] and got["volume"] == total[1]
    assert ref.CHUNK == 256


@pytest.mark.parametrize("bad", [1, 0, "yes", None, 1.0])
def test_mesh_stats_settings_refuses_what_is_not_a_bool(bad):
    from shapeclipper_amd.utils.util import EasyDict as edict
    from shapeclipper_amd.utils import options
    assert options.mesh_stats_settings(edict(eval=dict())) is False
    assert options.mesh_stats_settings(edict(eval=dict(mesh_stats=True))) is True
    assert options.mesh_stats_settings(edict(eval=dict(mesh_stats=False))) is False
    with pytest.raises(ValueError, match="eval.mesh_stats"):
        options.mesh_stats_settings(edict(eval=dict(mesh_stats=bad)))


def test_mesh_stats_is_not_a_hip_switch():
    from shapeclipper_amd.utils import options
    assert len(options.HIP_TABLE) == 35
    assert not any("mesh_stats" in str(row) for row in options.HIP_TABLE)


def test_line_of_mesh_stats_txt():
    import torch
    from shapeclipper_amd.utils.util import EasyDict as edict
    from shapeclipper_amd import ops
    from shapeclipper_amd.model import runner
    got = ref.mesh_topology(*MESHES["torus"][:2])
    stub = ops.MeshTopology(*(torch.tensor([got[k], 0]) for k in ref.INT_FIELDS), *(torch.tensor([got[k], True]) for k in ref.FLAGS),
                            torch.tensor([got["area"], 0.0], dtype=torch.float64), torch.tensor([got["volume"], 0.0], dtype=torch.float64),
                            torch.tensor(got["face_component"]))
    var = edict(idx=torch.tensor([7, 12]), category_label=torch.tensor([1, 0]), mesh_stats=stub._asdict())
    rec = runner._mesh_stats_records(var, "mesh_stats")
    assert rec.shape == (2, 20) and rec.dtype == torch.float64
    line = runner.mesh_stats_line(rec[0])
    assert line == "7 16 32 48 0 0 0 0 0 0 1 32 0 1 1 1 1 %.8f %.8f\n" % (got["area"], got["volume"])
    assert len(line.split()) == 19
    assert runner.mesh_stats_line(rec[1]).startswith("12 0 0 0 0 0 0 0 0 0 0 0 0 0 1 1 1 ")


def test_writers_of_mesh_stats_txt_and_mesh_stats_cat_txt(tmp_path):
    """Rows with the dual mesh's columns: the per-sample files (written anew, then appended to, as the vis_{ep}/ dump does) and the
    per-category files -- share of watertight-and-manifold samples, mean components, mean genus over the samples with genus >= 0."""
    import torch
    from shapeclipper_amd.utils.util import EasyDict as edict
    from shapeclipper_amd.model import runner
    keys = runner.MESH_STATS_KEYS
    assert len(keys) == 18 and runner.MESH_STATS_LINE.count("%") == 19

    def row(idx, cat, **kw):
        base = dict(dict.fromkeys(keys, 0), watertight=1, oriented=1, manifold=1, genus=-1)
        mc, dual = dict(base, **kw), dict(base, **{k[5:]: v for k, v in kw.items() if k.startswith("dual_")})
        return [idx] + [mc[k] for k in keys] + [cat] + [dual[k] for k in keys]
    rows = torch.tensor([row(3, 0, components=1, genus=0, area=1.5, volume=0.25, dual_components=2, dual_manifold=0),
                         row(5, 1, components=3, genus=2, dual_genus=1, dual_components=1),
                         row(8, 0, components=2, watertight=0, boundary_edges=7, dual_genus=3, dual_components=1)], dtype=torch.float64)
    assert rows.shape == (3, 38)
    runner._write_mesh_stats_lines(str(tmp_path), rows[:1])
    runner._write_mesh_stats_lines(str(tmp_path), rows[1:], "a")
    lines = open(tmp_path / "mesh_stats.txt").read().splitlines()
    assert lines[0] == "3 0 0 0 0 0 0 0 0 0 1 0 0 0 1 1 1 1.50000000 0.25000000" and [l.split()[0] for l in lines] == ["3", "5", "8"]
    assert lines[2].split()[4] == "7" and lines[2].split()[14] == "0"
    assert open(tmp_path / "mesh_stats_dual.txt").read().splitlines()[0] == "3 0 0 0 0 0 0 0 0 0 2 0 0 -1 1 1 0 0.00000000 0.00000000"
    runner._write_mesh_stats_lines(str(tmp_path), rows[:1, :20])               # without the dual columns: the one file, written anew
    assert len(open(tmp_path / "mesh_stats.txt").read().splitlines()) == 1
    assert len(open(tmp_path / "mesh_stats_dual.txt").read().splitlines()) == 3

    class Data:
        label2cat = {0: "chair", 1: "sofa"}

    class Stub:
        test_data = Data()
    o = edict(output_path=str(tmp_path), data=edict(num_classes=2))
    runner.Runner._write_mesh_stats(Stub(), o, rows)
    assert sorted(os.listdir(tmp_path)) == ["mesh_stats.txt", "mesh_stats_cat.txt", "mesh_stats_cat_dual.txt", "mesh_stats_dual.txt"]
    assert open(tmp_path / "mesh_stats_cat.txt").read().splitlines() == [
        "Closed Comps   Genus  Count Cat", "0.4998 1.4993 0.0000     2 chair", "0.9990 2.9970 1.9980     1 sofa"]
    assert open(tmp_path / "mesh_stats_cat_dual.txt").read().splitlines()[1:] == [
        "0.4998 1.4993 2.9970     2 chair", "0.9990 0.9990 0.9990     1 sofa"]
