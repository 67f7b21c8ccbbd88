"""`--mesh.subdivide=1` through Runner.evaluate and Runner.evaluate_sharded on the pix3d_mini tree (vox_res 16, 1000 points, four samples,
set up as tests/test_gpu_smooth_eval.py does), each into a clean folder: every sample with a mesh has {idx}_mesh_subdiv.ply with four
times the faces of {idx}_mesh.ply and an 18-field {idx}_mesh_subdiv.txt, in dump/ and in vis_{ep}/; the sharded run -- one sample at a
time, in a gloo process group of this one process -- writes the bytes of the unsharded one; two Newton steps against none change no face
and no fixed vertex and move no vertex farther than the clamp allows; a run without the switch writes no file of it and the chamfer.txt
of the runs with it; an architecture outside the compiled family runs the same steps on stock operators."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ARGS = ["--arch.enc_pretrained!", "--tb!", "--batch_size=2", "--data.pix3d.cat=chair,sofa", "--data.num_classes=2", "--data.num_workers=0",
        "--data.max_img_cat=2", "--eval.vox_res=16", "--eval.num_points=1000"]
FIELDS = ("idx levels project vertices_in vertices_out faces_in faces_out edges sharp_edges fixed resid_before resid_after disp_mean disp_max "
          "area_before area_after volume_before volume_after").split()
# two steps of at most 0.5 grid pitches each; the clamped step is 0.5 (1 + 2^-22) long at most and each subtraction rounds a coordinate
# below 32 by at most 2^-20 pitches: 2 * (0.5 + 2^-23 + sqrt(3) 2^-20) < 1 + 1e-5
MOVE_BOUND = 1.0 + 1e-5


def _ply_counts(fname):
    """(vertices, faces) of a PLY file's header."""
    head = open(fname, "rb").read(400).split(b"end_header")[0].decode("ascii").splitlines()
    return tuple(int([l for l in head if l.startswith("element " + e)][0].split()[2]) for e in ("vertex", "face"))


def _listing(path):
    return sorted(os.listdir(path)) + sorted(os.path.join("dump", f) for f in os.listdir(os.path.join(path, "dump")))


def _ours(path, folder="dump"):
    """{file name: bytes} of the *_mesh_subdiv.* files of a folder of the output path."""
    d = os.path.join(path, folder)
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if "_mesh_subdiv" in f}


def test_evaluation_writes_the_subdivided_meshes_and_their_sidecars(tmp_path):
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    import torch.distributed as dist
    from shapeclipper_amd.data import pix3d_mini
    from shapeclipper_amd.model.runner import Runner
    from shapeclipper_amd.utils import eval_3D, options
    from shapeclipper_amd.utils.util import EasyDict as edict
    tree = str(tmp_path / "Pix3D")
    pix3d_mini.write_tree(tree, n_per_cat=6, k_nearest=5, cat_key="chair,sofa", n_points=2000, seed=11)
    o = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_subdivide",
                                             "--output_root=%s" % (tmp_path / "out"), "--data.pix3d.root=%s" % tree, *ARGS,
                                             "--mesh.subdivide=1"]), verbose=False)
    o.device, o.world_size, o.port = 0, 1, 0
    torch.manual_seed(0)
    r = Runner(o)
    r.load_dataset(o, eval_split="test")
    r.build_networks(o)
    n = len(r.test_data)
    assert n == 4 and options.subdivide_settings(o) == (1, 2)
    seen = {}
    dump = r.dump_visuals

    def spy(opt, var, ep, train=False):
        """Keeps, per sample, the refined mesh in grid-index units with its fixed mask (None without the switch)."""
        for b, i in enumerate(var.idx.cpu().tolist()):
            seen[i] = None
            if "mesh_subdivided" in var and "mesh_subdivided_world" in var:
                m = var.mesh_subdivided
                v_end, f_end = (int(m[k][:b + 1].sum()) for k in ("v_count", "f_count"))
                nv, nf = int(m["v_count"][b]), int(m["f_count"][b])
                seen[i] = (m["verts"][v_end - nv:v_end].cpu().numpy(), m["faces"][f_end - nf:f_end].cpu().numpy(),
                           m["fixed"][v_end - nv:v_end].cpu().numpy())
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

    def check_files(res, project, folder="dump", samples=range(n)):
        n_meshes = 0
        for i in samples:
            d = os.path.join(res["path"], folder)
            line = open(os.path.join(d, "%d_mesh_subdiv.txt" % i)).read()
            assert line.endswith("\n") and line.count("\n") == 1
            f = dict(zip(FIELDS, line.split()))
            assert len(line.split()) == len(FIELDS) == 18 and int(f["idx"]) == i and int(f["levels"]) == 1 and int(f["project"]) == project
            assert int(f["faces_out"]) == 4 * int(f["faces_in"]) and int(f["vertices_out"]) == int(f["vertices_in"]) + int(f["edges"])
            print(folder, line.strip())
            plain, fine = (os.path.join(d, "%d_%s.ply" % (i, name)) for name in ("mesh", "mesh_subdiv"))
            assert os.path.exists(plain) == os.path.exists(fine)        # an empty mesh writes neither
            if os.path.exists(plain):
                assert _ply_counts(fine) == (int(f["vertices_out"]), 4 * _ply_counts(plain)[1]) and _ply_counts(plain)[1] == int(f["faces_in"])
                assert _ply_counts(plain)[0] == int(f["vertices_in"])
                reals = [float(f[k]) for k in FIELDS[10:]]
                if project:
                    assert np.isfinite(reals).all() and float(f["resid_before"]) >= 0 and 0.0 <= float(f["disp_mean"]) <= float(f["disp_max"])
                else:
                    assert f["resid_before"] == f["resid_after"] == "nan" and float(f["disp_mean"]) == 0.0 == float(f["disp_max"])
                    assert np.isfinite(reals[2:]).all()
                assert float(f["area_before"]) > 0 and float(f["area_after"]) > 0
                n_meshes += 1
        assert n_meshes >= 1

    plain = run("evaluate", "k2")
    check_files(plain, 2)
    # sharded, one sample at a time, inside a gloo process group (of this one process: the gather has nobody to wait for)
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        sharded = run("evaluate_sharded", "k2_sharded")
    finally:
        if created:
            dist.destroy_process_group()
    check_files(sharded, 2)
    assert sharded["listing"] == plain["listing"] and sharded["ours"] == plain["ours"] and len(plain["ours"]) >= 2
    # no Newton step: the same faces, the same fixed vertices, and the steps moved nothing farther than the clamp allows
    o.mesh.subdivide_project = 0
    bare = run("evaluate", "k0")
    check_files(bare, 0)
    assert bare["listing"] == plain["listing"] and bare["chamfer"] == plain["chamfer"] and bare["value"] == plain["value"]
    moved_any = False
    for i in range(n):
        (v2, f2, x2), (v0, f0, x0) = plain["meshes"][i], bare["meshes"][i]
        assert np.array_equal(f2, f0) and np.array_equal(x2, x0) and v2.shape == v0.shape
        assert np.array_equal(v2[x2].view(np.uint32), v0[x0].view(np.uint32))
        if len(v2):
            step = np.sqrt(((v2.astype(np.float64) - v0.astype(np.float64)) ** 2).sum(axis=1))
            print("sample %d: %d vertices, %d fixed, moved at most %.6f grid pitches" % (i, len(v2), int(x2.sum()), step.max()))
            assert step.max() <= MOVE_BOUND
            moved_any = moved_any or step.max() > 0
    assert moved_any
    # vis_{ep}/ of the training-time visualisation: the vis_only pass refines too and dump_geometry writes the same two files
    o.mesh.subdivide_project = 2
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
        assert "mesh_subdivided" in var and "mesh_subdivided_world" in var
        r.dump_geometry(o, var, "vis_3")
    i = int(var.idx[0])
    check_files(plain, 2, folder="vis_3", samples=[i])
    in_vis = _ours(o.output_path, "vis_3")
    assert in_vis and in_vis == {f: data for f, data in plain["ours"].items() if f.startswith("%d_" % i)}
    # the switch off: no file of it, nothing in var, the same chamfer.txt and the same returned value
    r.dump_visuals = spy
    del o.mesh.subdivide
    for mode in ("evaluate", "evaluate_sharded"):
        off = run(mode, mode + "_off")
        assert off["value"] == (plain if mode == "evaluate" else sharded)["value"]
        assert all(m is None for m in off["meshes"].values()) and not off["ours"]
        assert not [f for f in off["listing"] if "subdiv" in f]
        assert off["listing"] == [f for f in plain["listing"] if "subdiv" not in f]
        assert off["chamfer"] == plain["chamfer"] == sharded["chamfer"]


def test_an_architecture_outside_the_compiled_family_runs_on_stock_operators():
    from shapeclipper_amd.model.implicit import SDFNetwork
    from shapeclipper_amd.utils import eval_3D, options
    from shapeclipper_amd.utils.util import EasyDict as edict
    dev = torch.device("cuda:0")
    opt = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_subdivide_eager",
                                               "--output_root=/tmp/sc_pytest", "--arch.impl_sdf.n_channels=128", "--eval.vox_res=16",
                                               "--mesh.subdivide=2", "--mesh.subdivide_project=3"]), verbose=False)
    opt.device = dev
    torch.manual_seed(0)
    net = SDFNetwork(opt).to(dev)
    assert net.eager
    zs = torch.zeros(2, opt.arch.impl_sdf.proj_latent_dim, device=dev)
    runs = {}
    for k in (3, 0):
        opt.mesh.subdivide_project = k
        var = edict(idx=torch.arange(2, device=dev), proj_latent_sdf=zs)
        with torch.no_grad():
            var.level_vox = eval_3D.compute_level_grid(opt, net, zs, eval_3D.get_dense_3D_grid(opt, var))
            world = eval_3D.meshes_subdivided(opt, var, net)
        runs[k] = var.mesh_subdivided
        assert len(world) == 2 and len(eval_3D.subdivided_lines(var)) == 2 and all(len(l.split()) == 18 for l in eval_3D.subdivided_lines(var))
    fine, bare = runs[3], runs[0]
    assert int(fine["f_count"].sum()) > 0 and fine["f_count"].tolist() == [16 * int(c) for c in fine["faces_in"].tolist()]
    assert torch.equal(fine["faces"], bare["faces"]) and torch.equal(fine["fixed"], bare["fixed"])
    assert torch.equal(fine["verts"][fine["fixed"]].view(torch.int32), bare["verts"][bare["fixed"]].view(torch.int32))
    step = (fine["verts"].double() - bare["verts"].double()).norm(dim=1)
    assert 0 < float(step.max()) <= 3 * 0.5 + 1e-5                      # three steps of at most half a pitch (MOVE_BOUND's reasoning)
    assert torch.isfinite(fine["resid_before"]).all() and torch.isfinite(fine["resid_after"]).all() and torch.isnan(bare["resid_before"]).all()
    print("eager: resid %s -> %s, moved at most %.4f pitches" % (fine["resid_before"].tolist(), fine["resid_after"].tolist(), float(step.max())))
