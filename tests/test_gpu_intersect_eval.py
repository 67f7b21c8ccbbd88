"""`--mesh.self_intersect` through Runner.evaluate and Runner.evaluate_sharded on the pix3d_mini tree (vox_res 16, 1000 points, four
samples, set up as tests/test_gpu_subdivide_eval.py does) with every mesh variant switched on, each run into a clean folder: every sample
with a mesh has a five-line, 10-field {idx}_mesh_selfx.txt, in dump/ and in vis_{ep}/, whose counts are the numpy restatement's
(tests/mesh_intersect_ref.py) on the meshes the run held; {idx}_mesh_selfx_{variant}.ply exists exactly where faces_hit > 0; the sharded
run -- one sample at a time, in a gloo process group of this one process -- writes the bytes of the unsharded one; a run without the
switch writes none of these files and the same chamfer.txt."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_intersect_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ARGS = ["--arch.enc_pretrained!", "--tb!", "--batch_size=2", "--data.pix3d.cat=chair,sofa", "--data.num_classes=2", "--data.num_workers=0",
        "--data.max_img_cat=2", "--eval.vox_res=16", "--eval.num_points=1000"]
VARIANT_ARGS = ["--eval.dual_mesh", "--eval.simplify=2", "--mesh.smooth=3", "--mesh.subdivide=1"]
VARIANTS = ["mc", "dual", "simplified", "smooth", "subdiv"]
FIELDS = "idx variant faces degenerate box_pairs pairs pairs_vertex faces_hit first_face first_partner".split()


def _ply_counts(fname):
    """(vertices, faces) of a PLY file's header."""
    head = open(fname, "rb").read(400).split(b"end_header")[0].decode("ascii").splitlines()
    return tuple(int([l for l in head if l.startswith("element " + e)][0].split()[2]) for e in ("vertex", "face"))


def _listing(path):
    return sorted(os.listdir(path)) + sorted(os.path.join("dump", f) for f in os.listdir(os.path.join(path, "dump")))


def _ours(path, folder="dump"):
    """{file name: bytes} of the *_mesh_selfx* files of a folder of the output path."""
    d = os.path.join(path, folder)
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if "_mesh_selfx" in f}


def test_evaluation_writes_the_self_intersection_sidecars(tmp_path):
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    import torch.distributed as dist
    from shapeclipper_amd.data import pix3d_mini
    from shapeclipper_amd.model.runner import Runner
    from shapeclipper_amd.utils import eval_3D, options
    from shapeclipper_amd.utils.util import EasyDict as edict
    tree = str(tmp_path / "Pix3D")
    pix3d_mini.write_tree(tree, n_per_cat=6, k_nearest=5, cat_key="chair,sofa", n_points=2000, seed=11)
    o = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_selfx",
                                             "--output_root=%s" % (tmp_path / "out"), "--data.pix3d.root=%s" % tree, *ARGS, *VARIANT_ARGS,
                                             "--mesh.self_intersect"]), verbose=False)
    o.device, o.world_size, o.port = 0, 1, 0
    torch.manual_seed(0)
    r = Runner(o)
    r.load_dataset(o, eval_split="test")
    r.build_networks(o)
    n = len(r.test_data)
    assert n == 4 and options.self_intersect_settings(o) is True
    seen = {}
    dump = r.dump_visuals

    def spy(opt, var, ep, train=False):
        """Keeps, per sample, the meshes the check ran on, in grid-index units: {variant: (verts, faces)} (None without the switch)."""
        for b, i in enumerate(var.idx.cpu().tolist()):
            seen[i] = None
        if "mesh_intersections" in var:
            assert list(var.mesh_intersections) == VARIANTS
            for variant in var.mesh_intersections:
                per_image = eval_3D._intersection_meshes(var, variant).split()
                for b, i in enumerate(var.idx.cpu().tolist()):
                    seen[i] = seen[i] or {}
                    seen[i][variant] = tuple(t.cpu().numpy() for t in per_image[b])
        return dump(opt, var, ep, train=train)

    r.dump_visuals = spy

    def run(mode, name):
        o.output_path = str(tmp_path / "out" / name)                    # a clean folder each
        os.makedirs(o.output_path)
        seen.clear()
        value = getattr(r, mode)(o, ep=0)
        assert sorted(seen) == list(range(n))
        return dict(value=value, meshes=dict(seen), listing=_listing(o.output_path), ours=_ours(o.output_path), path=o.output_path,
                    chamfer=open(os.path.join(o.output_path, "chamfer.txt"), "rb").read())

    want = {}

    def restated(i, variant, mesh):
        if (i, variant) not in want:
            w = ref.image_self_intersections(*mesh)
            hit = np.flatnonzero(w["hits"] > 0)
            first = int(hit[0]) if len(hit) else -1
            want[(i, variant)] = [len(mesh[1]), w["degenerate"], w["box_pairs"], w["pairs"], w["pairs_vertex"], w["faces_hit"], first,
                                  int(w["partner"][first]) if first >= 0 else -1]
        return want[(i, variant)]

    def check_files(res, folder="dump", samples=range(n)):
        n_meshes = 0
        for i in samples:
            d = os.path.join(res["path"], folder)
            text = open(os.path.join(d, "%d_mesh_selfx.txt" % i)).read()
            assert text.endswith("\n") and text.count("\n") == 5
            for line, variant in zip(text.splitlines(), VARIANTS):
                f = dict(zip(FIELDS, line.split()))
                assert len(line.split()) == len(FIELDS) == 10 and int(f["idx"]) == i and f["variant"] == variant
                print(folder, line)
                got = [int(f[k]) for k in FIELDS[2:]]
                assert got == restated(i, variant, res["meshes"][i][variant]), (i, variant)
                assert os.path.exists(os.path.join(d, "%d_mesh_selfx_%s.ply" % (i, variant))) == (int(f["faces_hit"]) > 0)
                if int(f["faces_hit"]) > 0:
                    assert _ply_counts(os.path.join(d, "%d_mesh_selfx_%s.ply" % (i, variant)))[1] == int(f["faces_hit"])
                if variant == "mc" and os.path.exists(os.path.join(d, "%d_mesh.ply" % i)):
                    assert _ply_counts(os.path.join(d, "%d_mesh.ply" % i))[1] == int(f["faces"])
                    n_meshes += 1
                if variant == "subdiv":
                    assert int(f["faces"]) == 4 * int(text.splitlines()[0].split()[2])
        assert n_meshes >= 1

    plain = run("evaluate", "on")
    check_files(plain)
    # sharded, one sample at a time, inside a gloo process group (of this one process: the gather has nobody to wait for)
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        sharded = run("evaluate_sharded", "on_sharded")
    finally:
        if created:
            dist.destroy_process_group()
    check_files(sharded)
    assert sharded["listing"] == plain["listing"] and sharded["ours"] == plain["ours"] and len(plain["ours"]) >= n
    # vis_{ep}/ of the training-time visualisation: the vis_only pass checks too and dump_geometry writes the same files
    r.dump_visuals = dump
    r.graph.eval()
    o.H, o.W = o.eval.image_size
    o.output_path = plain["path"]
    os.makedirs(os.path.join(o.output_path, "vis_3"), exist_ok=True)
    sample = r.test_data[0]
    batch = {key: ({kk: vv[None] for kk, vv in v.items()} if isinstance(v, dict) else torch.as_tensor(v)[None]) for key, v in sample.items()}
    with torch.no_grad():
        var = r.evaluate_batch(o, edict(batch), 0, 0, single_gpu=True)
        eval_3D.eval_metrics(o, var, r.graph.module.sdf_network, vis_only=True)
        assert "mesh_intersections" in var and list(var.mesh_intersections) == VARIANTS
        r.dump_geometry(o, var, "vis_3")
    i = int(var.idx[0])
    check_files(plain, folder="vis_3", samples=[i])
    in_vis = _ours(o.output_path, "vis_3")
    assert in_vis and in_vis == {f: data for f, data in plain["ours"].items() if f.startswith("%d_" % i)}
    # the switch off: no file of it, nothing in var, the same chamfer.txt and the same returned value
    r.dump_visuals = spy
    del o.mesh.self_intersect
    for mode in ("evaluate", "evaluate_sharded"):
        off = run(mode, mode + "_off")
        assert off["value"] == (plain if mode == "evaluate" else sharded)["value"]
        assert all(m is None for m in off["meshes"].values()) and not off["ours"]
        assert not [f for f in off["listing"] if "selfx" in f]
        assert off["listing"] == [f for f in plain["listing"] if "selfx" not in f]
        assert off["chamfer"] == plain["chamfer"] == sharded["chamfer"]


def test_only_the_written_variants_are_checked_and_hit_faces_are_written(tmp_path):
    """eval_3D.mesh_intersections on two hand-made level grids, without a network: the marching-cubes variant alone, no hit and no
    file; then the same var with two crossing spheres in the place of a simplified mesh, whose hit faces are written."""
    from shapeclipper_amd import ops
    from shapeclipper_amd.utils import eval_3D, options, util_vis
    from shapeclipper_amd.utils.util import EasyDict as edict
    import mesh_simplify_ref
    dev = torch.device("cuda:0")
    opt = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_selfx_hand",
                                               "--output_root=%s" % tmp_path, "--mesh.self_intersect"]), verbose=False)
    os.makedirs(os.path.join(opt.output_path, "dump"), exist_ok=True)
    level = torch.as_tensor(np.stack([mesh_simplify_ref.level("sphere"), mesh_simplify_ref.level("torus")])).to(dev)
    var = edict(idx=torch.tensor([7, 9], device=dev), level_vox=level)
    out = eval_3D.mesh_intersections(opt, var)
    assert list(out) == ["mc"] and out["mc"]["pairs"].tolist() == [0, 0] and out["mc"]["f_count"].tolist() == [1088, 1056]
    assert out["mc"]["box_pairs"].tolist() == [6423, 6400]              # the restatement's figures on these two meshes (host test)
    lines = eval_3D.intersection_lines(var)
    assert lines == ["7 mc 1088 0 6423 0 0 0 -1 -1", "9 mc 1056 0 6400 0 0 0 -1 -1"]
    assert eval_3D.intersection_hit_meshes(opt, var, "mc") == ([], [])
    # a "simplified" mesh that does cross itself: image 0 the two spheres, image 1 nothing
    v, f = ref.two_spheres()
    var.mesh_simplified = dict(verts=torch.as_tensor(v).to(dev), faces=torch.as_tensor(f).to(dev), v_count=torch.tensor([len(v), 0]),
                               f_count=torch.tensor([len(f), 0]))
    out = eval_3D.mesh_intersections(opt, var)
    w = ref.image_self_intersections(v, f)
    assert list(out) == ["mc", "simplified"] and out["simplified"]["pairs"].tolist() == [w["pairs"], 0] and w["pairs"] > 0
    first = int(np.flatnonzero(w["hits"] > 0)[0])
    assert eval_3D.intersection_lines(var)[0].splitlines()[1] == "7 simplified %d 0 %d %d 0 %d %d %d" % (
        len(f), w["box_pairs"], w["pairs"], w["faces_hit"], first, int(w["partner"][first]))
    assert eval_3D.intersection_lines(var)[1].splitlines()[1] == "9 simplified 0 0 0 0 0 0 -1 -1"
    rows, meshes = eval_3D.intersection_hit_meshes(opt, var, "simplified")
    assert rows == [0] and meshes[0][1].shape == (w["faces_hit"], 3) and meshes[0][1].dtype == torch.int32
    lo, hi = opt.eval.range
    hit_faces = f[w["hits"] > 0]
    used = np.unique(hit_faces)
    assert int(meshes[0][1].max()) == len(used) - 1 and meshes[0][0].shape == (len(used), 3)
    expect = eval_3D.written_position(torch.as_tensor(v[used]).to(dev), lo, hi, 17)
    assert torch.equal(meshes[0][0], expect)
    assert np.array_equal(used[meshes[0][1].cpu().numpy()], hit_faces)
    util_vis.dump_meshes(opt, [var.idx[b] for b in rows], "mesh_selfx_simplified", meshes)
    assert _ply_counts(os.path.join(opt.output_path, "dump", "7_mesh_selfx_simplified.ply")) == (len(used), w["faces_hit"])
    assert not os.path.exists(os.path.join(opt.output_path, "dump", "9_mesh_selfx_simplified.ply"))
