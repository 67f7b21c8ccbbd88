"""`--mesh.smooth=5` through Runner.evaluate and Runner.evaluate_sharded on the pix3d_mini tree (vox_res 16, 1000 points, four samples,
set up as tests/test_gpu_eval_all_reports.py does), each into a clean folder: both list the same files, every sample has
{idx}_mesh_smooth.ply with the faces of {idx}_mesh.ply and a 17-field {idx}_mesh_smooth.txt that is the same line in both modes, and
chamfer.txt has the bytes of a run without the switch -- which writes no *_smooth* file and leaves no "mesh_smoothed" in var."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ARGS = ["--arch.enc_pretrained!", "--tb!", "--batch_size=2", "--data.pix3d.cat=chair,sofa", "--data.num_classes=2", "--data.num_workers=0",
        "--data.max_img_cat=2", "--eval.vox_res=16", "--eval.num_points=1000"]
FIELDS = ("idx iters lambda mu vertices free fixed_boundary isolated degree_max disp_mean disp_max rough_before rough_after area_before "
          "area_after volume_before volume_after").split()


def _ply_counts(fname):
    """(vertices, faces) of a PLY file's header."""
    head = open(fname, "rb").read(400).split(b"end_header")[0].decode("ascii").splitlines()
    return tuple(int([l for l in head if l.startswith("element " + e)][0].split()[2]) for e in ("vertex", "face"))


def _listing(path):
    return sorted(os.listdir(path)) + sorted(os.path.join("dump", f) for f in os.listdir(os.path.join(path, "dump")))


def test_evaluation_writes_the_smoothed_meshes_and_their_sidecars(tmp_path):
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    from shapeclipper_amd.data import pix3d_mini
    from shapeclipper_amd.model.runner import Runner
    from shapeclipper_amd.utils import options
    tree = str(tmp_path / "Pix3D")
    pix3d_mini.write_tree(tree, n_per_cat=6, k_nearest=5, cat_key="chair,sofa", n_points=2000, seed=11)
    o = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_smooth",
                                             "--output_root=%s" % (tmp_path / "out"), "--data.pix3d.root=%s" % tree, *ARGS,
                                             "--mesh.smooth=5"]), verbose=False)
    o.device, o.world_size, o.port = 0, 1, 0
    torch.manual_seed(0)
    r = Runner(o)
    r.load_dataset(o, eval_split="test")
    r.build_networks(o)
    n = len(r.test_data)
    assert n == 4
    seen = []
    dump = r.dump_visuals

    def spy(opt, var, ep, train=False):
        seen.append("mesh_smoothed" in var and "mesh_smoothed_world" in var)
        return dump(opt, var, ep, train=train)

    r.dump_visuals = spy
    lines, listing, chamfer, values = {}, {}, {}, {}
    for mode in ("evaluate", "evaluate_sharded"):
        o.output_path = str(tmp_path / "out" / mode)                    # a clean folder each
        os.makedirs(o.output_path)
        seen.clear()
        values[mode] = getattr(r, mode)(o, ep=0)
        assert seen and all(seen)
        listing[mode] = _listing(o.output_path)
        chamfer[mode] = open(os.path.join(o.output_path, "chamfer.txt"), "rb").read()
        lines[mode] = {}
        n_meshes = 0
        for i in range(n):
            dump_dir = os.path.join(o.output_path, "dump")
            line = open(os.path.join(dump_dir, "%d_mesh_smooth.txt" % i)).read()
            assert line.endswith("\n") and line.count("\n") == 1
            f = dict(zip(FIELDS, line.split()))
            assert len(line.split()) == len(FIELDS) == 17 and int(f["idx"]) == i and int(f["iters"]) == 5
            assert float(f["lambda"]) == 0.5 and float(f["mu"]) == 1.0 / (0.1 - 2.0)
            assert int(f["free"]) + int(f["fixed_boundary"]) + int(f["isolated"]) == int(f["vertices"])
            print(mode, line.strip())
            plain, smooth = (os.path.join(dump_dir, "%d_%s.ply" % (i, name)) for name in ("mesh", "mesh_smooth"))
            assert os.path.exists(plain) == os.path.exists(smooth)      # an empty mesh writes neither
            if os.path.exists(plain):
                assert _ply_counts(smooth) == _ply_counts(plain) and _ply_counts(smooth)[0] == int(f["vertices"])
                assert 0.0 <= float(f["disp_mean"]) <= float(f["disp_max"]) and float(f["area_before"]) > 0 and float(f["area_after"]) > 0
                assert np.isfinite([float(x) for x in line.split()]).all()
                n_meshes += 1
            lines[mode][i] = line
        assert n_meshes >= 1, mode
    assert listing["evaluate"] == listing["evaluate_sharded"]
    assert lines["evaluate"] == lines["evaluate_sharded"]
    # the switch off: no file of it, nothing in var, the same chamfer.txt and the same returned value
    del o.mesh.smooth
    for mode in ("evaluate", "evaluate_sharded"):
        o.output_path = str(tmp_path / "out" / (mode + "_off"))
        os.makedirs(o.output_path)
        seen.clear()
        assert getattr(r, mode)(o, ep=0) == values[mode]
        assert seen and not any(seen)
        off = _listing(o.output_path)
        assert not [f for f in off if "smooth" in f]
        assert off == [f for f in listing[mode] if "smooth" not in f]
        assert open(os.path.join(o.output_path, "chamfer.txt"), "rb").read() == chamfer[mode]
