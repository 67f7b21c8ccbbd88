"""Every optional evaluation output at once on the pix3d_mini tree (vox_res 16, 1000 points, four samples, two categories, seeded
weights): Runner.evaluate and Runner.evaluate_sharded, each into a clean folder, write the same file names, the same bytes in every
.txt that both form from the per-sample records, and one line per sample, with the field count of its line format, in every
per-sample .txt.  The sha256 of every .txt is printed, so that two versions of the host plumbing can be compared file by file."""
import hashlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ARGS = ["--arch.enc_pretrained!", "--tb!", "--batch_size=2", "--data.pix3d.cat=chair,sofa", "--data.num_classes=2", "--data.num_workers=0",
        "--data.max_img_cat=2", "--eval.vox_res=16", "--eval.num_points=1000",
        "--eval.icp", "--eval.normals", "--eval.mesh_dist", "--eval.dual_mesh", "--eval.emd", "--eval.emd_points=64", "--eval.iou",
        "--eval.mesh_stats", "--eval.simplify=2", "--eval.texture", "--eval.texture_texels=4", "--eval.mesh_render", "--hip.largest_component"]
# per-sample file -> the name of its line format in utils/eval_reports.py, or its field count where the line is written in place
PER_SAMPLE = {"chamfer.txt": 3, "chamfer_icp.txt": 3, "icp.txt": 6, "components.txt": 4,
              "normal_consistency.txt": "NC_LINE", "normal_consistency_icp.txt": "NC_LINE",
              "completeness_mesh.txt": "MESH_LINE", "completeness_mesh_dual.txt": "MESH_LINE",
              "emd.txt": "EMD_LINE", "emd_icp.txt": "EMD_LINE", "iou.txt": "IOU_LINE", "iou_icp.txt": "IOU_LINE",
              "mesh_stats.txt": "MESH_STATS_LINE", "mesh_stats_dual.txt": "MESH_STATS_LINE", "mesh_stats_simplified.txt": "MESH_STATS_LINE",
              "simplify.txt": "SIMPLIFY_LINE", "texture.txt": "TEXTURE_LINE", "mesh_render.txt": "MESH_RENDER_LINE"}
TABLES = ("cd_cat.txt", "f_score.txt", "cd_cat_icp.txt", "f_score_icp.txt", "nc_cat.txt", "nc_cat_icp.txt", "cd_cat_mesh.txt",
          "cd_cat_mesh_dual.txt", "f_score_mesh.txt", "f_score_mesh_dual.txt", "emd_cat.txt", "emd_cat_icp.txt", "iou_cat.txt",
          "iou_cat_icp.txt", "mesh_stats_cat.txt", "mesh_stats_cat_dual.txt")
# evaluate() tallies these four from .item() values in Python floats, evaluate_sharded sums fp32 rows: the same values, another
# arithmetic, so a fourth decimal may differ.  Every other .txt is formed from the same float64 records by the same code.
OTHER_ARITHMETIC = ("cd_cat.txt", "f_score.txt", "cd_cat_icp.txt", "f_score_icp.txt")


def _texts(path):
    return {f: open(os.path.join(path, f), "rb").read() for f in sorted(os.listdir(path)) if f.endswith(".txt")}


def test_evaluate_and_evaluate_sharded_write_the_same_reports(tmp_path):
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    from shapeclipper_amd.data import pix3d_mini
    from shapeclipper_amd.model.runner import Runner
    from shapeclipper_amd.utils import eval_reports, options
    tree = str(tmp_path / "Pix3D")
    pix3d_mini.write_tree(tree, n_per_cat=6, k_nearest=5, cat_key="chair,sofa", n_points=2000, seed=11)
    o = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_all_reports",
                                             "--output_root=%s" % (tmp_path / "out"), "--data.pix3d.root=%s" % tree, *ARGS]), verbose=False)
    o.device, o.world_size, o.port = 0, 1, 0
    torch.manual_seed(0)
    r = Runner(o)
    r.load_dataset(o, eval_split="test")
    r.build_networks(o)
    n = len(r.test_data)
    assert n == 4 and o.data.num_classes == 2
    out, listing = {}, {}
    for mode in ("evaluate", "evaluate_sharded"):
        o.output_path = str(tmp_path / "out" / mode)                    # a clean folder each
        os.makedirs(o.output_path)
        getattr(r, mode)(o, ep=0)
        out[mode] = _texts(o.output_path)
        listing[mode] = sorted(os.listdir(o.output_path)) + sorted(os.listdir(os.path.join(o.output_path, "dump")))
        for f, data in out[mode].items():
            print("%s  %s/%s" % (hashlib.sha256(data).hexdigest(), mode, f))
    single, sharded = out["evaluate"], out["evaluate_sharded"]
    assert listing["evaluate"] == listing["evaluate_sharded"]
    assert sorted(single) == sorted(tuple(PER_SAMPLE) + TABLES)
    for mode, files in out.items():
        ids = [l.split()[0] for l in files["chamfer.txt"].decode().splitlines()]
        assert ids == [str(i) for i in range(n)]
        for f, line in PER_SAMPLE.items():
            fields = line if isinstance(line, int) else getattr(eval_reports, line).count("%")
            rows = [l.split() for l in files[f].decode().splitlines()]
            assert [row[0] for row in rows] == ids and all(len(row) == fields for row in rows), (mode, f, rows)
    differ = [f for f in single if single[f] != sharded[f]]
    print("files that differ between evaluate and evaluate_sharded:", differ)
    if single["chamfer.txt"] == sharded["chamfer.txt"]:
        assert [f for f in differ if f not in OTHER_ARITHMETIC] == []
    else:
        print("evaluate and evaluate_sharded differ on chamfer.txt: the other files are not compared")
