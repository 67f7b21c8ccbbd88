"""`--mesh.decimate=60` through Runner.evaluate and Runner.evaluate_sharded on the pix3d_mini tree (vox_res 16, 1000 points, four samples,
set up as tests/test_gpu_smooth_eval.py does), each into a clean folder: both list the same files, every sample has
{idx}_mesh_decimated.ply and an 18-field {idx}_mesh_decimated.txt whose numbers are those of a direct ops.mesh_decimate call on the
sample's own marching-cubes mesh, the PLY overlays {idx}_mesh.ply, the vis_{ep}/ dump of the training-time visualisation writes the same
two files, `--mesh.self_intersect` gets a last line `decimated`, and a run without the switch lists the same files and has the bytes of
chamfer.txt and {idx}_mesh.ply of a run with it -- and writes no *_decimated* file and leaves no "mesh_decimated" in var."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ARGS = ["--arch.enc_pretrained!", "--tb!", "--batch_size=2", "--data.pix3d.cat=chair,sofa", "--data.num_classes=2", "--data.num_workers=0",
        "--data.max_img_cat=2", "--eval.vox_res=16", "--eval.num_points=1000"]
FIELDS = ("idx target vertices_in vertices_out faces_in faces_out rounds collapses rejected_link rejected_flip fixed reached dist_mean "
          "dist_max area_before area_after volume_before volume_after").split()
TARGET = 60


def _ply(fname):
    """(vertices [V,3] float32, face count) of a binary PLY whose vertex element is x y z."""
    data = open(fname, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    nv, nf = (int([l for l in lines if l.startswith("element " + e)][0].split()[2]) for e in ("vertex", "face"))
    return np.frombuffer(body[:12 * nv], "<f4").reshape(nv, 3), nf


def _listing(path):
    return sorted(os.listdir(path)) + sorted(os.path.join("dump", f) for f in os.listdir(os.path.join(path, "dump")))


def _files(path, pick, folder="dump"):
    d = os.path.join(path, folder)
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if pick(f)}


def test_evaluation_writes_the_decimated_meshes_and_their_sidecars(tmp_path):
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    import torch.distributed as dist
    from shapeclipper_amd import ops
    from shapeclipper_amd.data import pix3d_mini
    from shapeclipper_amd.model.runner import Runner
    from shapeclipper_amd.utils import eval_3D, options
    from shapeclipper_amd.utils.util import EasyDict as edict
    tree = str(tmp_path / "Pix3D")
    pix3d_mini.write_tree(tree, n_per_cat=6, k_nearest=5, cat_key="chair,sofa", n_points=2000, seed=11)
    o = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_decimate",
                                             "--output_root=%s" % (tmp_path / "out"), "--data.pix3d.root=%s" % tree, *ARGS,
                                             "--mesh.decimate=%d" % TARGET]), verbose=False)
    o.device, o.world_size, o.port = 0, 1, 0
    torch.manual_seed(0)
    r = Runner(o)
    r.load_dataset(o, eval_split="test")
    r.build_networks(o)
    n = len(r.test_data)
    assert n == 4 and options.decimate_settings(o) == (TARGET, 1e-3, 1024)
    lo, hi = o.eval.range
    seen = {}
    dump = r.dump_visuals

    def spy(opt, var, ep, train=False):
        """Keeps, per sample, its marching-cubes mesh in grid-index units and whether the decimated one is in var."""
        held = "mesh_decimated" in var and "mesh_decimated_world" in var
        per_image = ops.PackedMesh(*var.mesh_packed).split() if "mesh_packed" in var else [None] * len(var.idx)
        for b, i in enumerate(var.idx.cpu().tolist()):
            seen[i] = (held, per_image[b], var.level_vox.shape[1])
        return dump(opt, var, ep, train=train)

    r.dump_visuals = spy

    def run(mode, name):
        o.output_path = str(tmp_path / "out" / name)                    # a clean folder each
        os.makedirs(o.output_path)
        seen.clear()
        value = getattr(r, mode)(o, ep=0)
        assert sorted(seen) == list(range(n))
        return dict(value=value, seen=dict(seen), listing=_listing(o.output_path), path=o.output_path,
                    ours=_files(o.output_path, lambda f: "_mesh_decimated" in f),
                    plain=_files(o.output_path, lambda f: f.endswith("_mesh.ply")),
                    chamfer=open(os.path.join(o.output_path, "chamfer.txt"), "rb").read())

    def check_files(res, folder="dump", samples=range(n)):
        n_meshes = 0
        for i in samples:
            d = os.path.join(res["path"], folder)
            line = open(os.path.join(d, "%d_mesh_decimated.txt" % i)).read()
            assert line.endswith("\n") and line.count("\n") == 1
            f = dict(zip(FIELDS, line.split()))
            assert len(line.split()) == len(FIELDS) == 18 and int(f["idx"]) == i and int(f["target"]) == TARGET
            print(folder, line.strip())
            held, (verts, faces), S = res["seen"][i]
            assert held and int(f["vertices_in"]) == len(verts) and int(f["faces_in"]) == len(faces)
            plain, few = (os.path.join(d, "%d_%s.ply" % (i, name)) for name in ("mesh", "mesh_decimated"))
            assert os.path.exists(plain) == os.path.exists(few)         # an empty mesh writes neither
            # the numbers of a direct call on the sample's own mesh
            direct = ops.mesh_decimate(verts.contiguous(), faces.contiguous(), torch.tensor([len(verts)]), torch.tensor([len(faces)]), TARGET)
            assert [int(f[k]) for k in FIELDS[3:12:1] if k != "faces_in"] == [
                int(direct.v_count[0]), int(direct.f_count[0]), int(direct.rounds[0]), int(direct.collapses[0]), int(direct.rejected_link[0]),
                int(direct.rejected_flip[0]), int(direct.fixed_vertices[0]), int(direct.reached[0])]
            if os.path.exists(plain):
                to_object = lambda v: eval_3D.sampled_position(v, lo, hi, S).contiguous()
                dist2 = ops.point_mesh_distance(to_object(verts)[None].contiguous(), to_object(direct.verts), direct.faces, direct.v_count,
                                                direct.f_count).dist2
                # the maximum is exact; the fp32 mean of N <= 2^12 values is summed in the batch's order there: within N 2^-24 < 2.5e-4
                assert f["dist_max"] == "%.9g" % float(dist2.sqrt().max())
                assert abs(float(f["dist_mean"]) - float(dist2.sqrt().mean())) <= 2.5e-4 * float(dist2.sqrt().mean())
                before = ops.mesh_topology(to_object(verts), faces.contiguous(), torch.tensor([len(verts)]), torch.tensor([len(faces)]))
                after = ops.mesh_topology(*direct.packed._replace(verts=to_object(direct.verts)))
                assert [f[k] for k in FIELDS[14:]] == ["%.9g" % float(x[0]) for x in (before.area, after.area, before.volume, after.volume)]
                # the PLY: the op's vertices with {idx}_mesh.ply's rescale, inside that mesh's box
                pv, pf = _ply(few)
                mv, mf = _ply(plain)
                assert (len(pv), pf) == (int(f["vertices_out"]), int(f["faces_out"])) and (len(mv), mf) == (len(verts), len(faces))
                want = eval_3D.written_position(direct.verts, lo, hi, S).cpu().numpy().astype(np.float32)
                assert np.array_equal(pv.view(np.uint32), want.view(np.uint32))
                assert (pv.min(axis=0) >= mv.min(axis=0) - 1.0 / S).all() and (pv.max(axis=0) <= mv.max(axis=0) + 1.0 / S).all()
                if len(faces) > TARGET:
                    assert int(f["faces_out"]) < int(f["faces_in"]) and int(f["collapses"]) >= 1 and int(f["rounds"]) >= 1
                    assert int(f["faces_out"]) == int(f["faces_in"]) - 2 * int(f["collapses"])
                    assert float(f["dist_max"]) >= float(f["dist_mean"]) >= 0.0
                else:
                    assert np.array_equal(pv.view(np.uint32), mv.view(np.uint32)) and int(f["rounds"]) == 0 and int(f["reached"]) == 1
                n_meshes += 1
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
    assert sharded["listing"] == plain["listing"] and sharded["ours"] == plain["ours"] and len(plain["ours"]) >= n + 1
    # vis_{ep}/ of the training-time visualisation: the vis_only pass decimates too and dump_geometry writes the same two files
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
        assert "mesh_decimated" in var and "mesh_decimated_world" in var
        r.dump_geometry(o, var, "vis_3")
    i = int(var.idx[0])
    in_vis = _files(o.output_path, lambda f: "_mesh_decimated" in f, "vis_3")
    assert in_vis and in_vis == {f: data for f, data in plain["ours"].items() if f.startswith("%d_" % i)}
    # with --mesh.self_intersect as well: `decimated` is the last line
    r.dump_visuals = spy
    o.mesh.self_intersect = True
    both = run("evaluate", "with_selfx")
    for i in range(n):
        text = open(os.path.join(both["path"], "dump", "%d_mesh_selfx.txt" % i)).read().splitlines()
        assert [l.split()[1] for l in text] == ["mc", "decimated"] and int(text[1].split()[0]) == i
        few = open(os.path.join(both["path"], "dump", "%d_mesh_decimated.txt" % i)).read().split()
        assert int(text[1].split()[2]) == int(few[FIELDS.index("faces_out")])
    assert both["ours"] == plain["ours"]
    del o.mesh.self_intersect
    # the switch off: no file of it, nothing in var, the same listing otherwise, the same chamfer.txt, {idx}_mesh.ply and returned value
    del o.mesh.decimate
    for mode in ("evaluate", "evaluate_sharded"):
        off = run(mode, mode + "_off")
        assert off["value"] == (plain if mode == "evaluate" else sharded)["value"]
        assert not any(held for held, _, _ in off["seen"].values()) and not off["ours"]
        assert not [f for f in off["listing"] if "decimated" in f]
        assert off["listing"] == [f for f in plain["listing"] if "decimated" not in f]
        assert off["chamfer"] == plain["chamfer"] == sharded["chamfer"]
        assert off["plain"] == plain["plain"] and len(off["plain"]) >= 1
