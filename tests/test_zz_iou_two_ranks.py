"""`evaluate.py --eval.iou` on the pix3d_mini tree in one process and under the launcher with two ranks.  A file of its own, named to sort
behind every kernel test: tests that start other processes must not stand in front of a kernel-against-restatement test
(tests/conftest.py orders the suite by file; tests/test_host_logic.py holds every test_gpu_*.py file outside the last group to that)."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
IOU_FILES = ("iou.txt", "iou_cat.txt", "iou_icp.txt", "iou_cat_icp.txt")
TREE_ARGS = ["--arch.enc_pretrained!", "--tb!", "--batch_size=2", "--data.pix3d.cat=chair,sofa", "--data.num_classes=2", "--data.num_workers=0",
             "--data.max_img_cat=2", "--eval.vox_res=16", "--eval.num_points=1000"]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from shapeclipper_amd.data import pix3d_mini
    root = str(tmp_path_factory.mktemp("pix3d_iou_ranks") / "Pix3D")
    pix3d_mini.write_tree(root, n_per_cat=6, k_nearest=5, cat_key="chair,sofa", n_points=2000, seed=11)
    return root


def test_two_gloo_ranks_of_evaluate_py_write_the_unsharded_lines(tree, tmp_path):
    """evaluate.py with --eval.iou --eval.iou_res=24 --eval.icp on the pix3d_mini tree (seeded random weights, no checkpoint) in one
    process and under the launcher with two ranks on the one GPU over gloo: rank 0's extra gather gives the four files of the single
    process, byte for byte."""
    import socket
    import subprocess
    args = ["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=iou_e2e", "--output_root=%s" % tmp_path, "--data.pix3d.root=%s" % tree,
            *TREE_ARGS, "--eval.iou", "--eval.iou_res=24", "--eval.icp"]
    env = dict(os.environ, MIOPEN_LOG_LEVEL="1", MIOPEN_FIND_MODE="FAST", SHAPECLIPPER_DIST_BACKEND="gloo")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = os.path.join(str(tmp_path), "pix3d_output", "iou_e2e")

    def run(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        got = {f: open(os.path.join(out, f), "rb").read() for f in IOU_FILES + ("chamfer.txt",)}
        for f in got:
            os.remove(os.path.join(out, f))
        return got

    single = run([sys.executable, os.path.join(ROOT, "evaluate.py")] + args)
    sharded = run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                   "--master-port", str(port), os.path.join(ROOT, "evaluate.py")] + args)
    print(single["iou.txt"].decode())
    lines = single["iou.txt"].decode().splitlines()
    assert len(lines) == 4 and all(len(l.split()) == 9 and l.split()[1] == "24" for l in lines)
    for f in IOU_FILES:
        assert sharded[f] == single[f], (f, single[f], sharded[f])
