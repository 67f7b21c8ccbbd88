"""`evaluate.py --eval.mesh_stats --eval.dual_mesh` on the pix3d_mini tree in one process and under the launcher with two ranks.  A file of
its own, named to sort behind every kernel test: tests that start other processes must not stand in front of a kernel-against-restatement
test (tests/conftest.py orders the suite by file; tests/test_host_logic.py holds every test_gpu_*.py file outside the last group to that)."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
STATS_FILES = ("mesh_stats.txt", "mesh_stats_dual.txt", "mesh_stats_cat.txt", "mesh_stats_cat_dual.txt")
TREE_ARGS = ["--arch.enc_pretrained!", "--tb!", "--batch_size=2", "--data.pix3d.cat=chair,sofa", "--data.num_classes=2", "--data.num_workers=0",
             "--data.max_img_cat=2", "--eval.vox_res=16", "--eval.num_points=1000"]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from shapeclipper_amd.data import pix3d_mini
    root = str(tmp_path_factory.mktemp("pix3d_stats_ranks") / "Pix3D")
    pix3d_mini.write_tree(root, n_per_cat=6, k_nearest=5, cat_key="chair,sofa", n_points=2000, seed=11)
    return root


def test_two_gloo_ranks_of_evaluate_py_write_the_unsharded_lines(tree, tmp_path):
    """evaluate.py with --eval.mesh_stats --eval.dual_mesh on the pix3d_mini tree (seeded random weights, no checkpoint) in one process
    and under the launcher with two ranks on the one GPU over gloo: rank 0's extra gather gives the files of the single process, byte
    for byte; mesh_stats.txt has one line of 19 fields per sample; chamfer.txt is that of a run without the switch."""
    import socket
    import subprocess
    args = ["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=stats_e2e", "--output_root=%s" % tmp_path, "--data.pix3d.root=%s" % tree,
            *TREE_ARGS]
    on = ["--eval.mesh_stats", "--eval.dual_mesh"]
    env = dict(os.environ, MIOPEN_LOG_LEVEL="1", MIOPEN_FIND_MODE="FAST", SHAPECLIPPER_DIST_BACKEND="gloo")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = os.path.join(str(tmp_path), "pix3d_output", "stats_e2e")

    def run(cmd, files):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        got = {f: open(os.path.join(out, f), "rb").read() for f in files}
        listing = sorted(os.listdir(out))
        for f in listing:
            if f in got or f.startswith("mesh_stats"):
                os.remove(os.path.join(out, f))
        return got, listing

    single, _ = run([sys.executable, os.path.join(ROOT, "evaluate.py")] + args + on, STATS_FILES + ("chamfer.txt",))
    sharded, _ = run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                      "--master-port", str(port), os.path.join(ROOT, "evaluate.py")] + args + on, STATS_FILES + ("chamfer.txt",))
    off, listing = run([sys.executable, os.path.join(ROOT, "evaluate.py")] + args, ("chamfer.txt",))
    print(single["mesh_stats.txt"].decode(), single["mesh_stats_dual.txt"].decode(), single["mesh_stats_cat.txt"].decode(), sep="\n")
    for name in ("mesh_stats.txt", "mesh_stats_dual.txt"):
        lines = single[name].decode().splitlines()
        assert len(lines) == 4 and all(len(l.split()) == 19 for l in lines), lines
    assert [l.split()[0] for l in single["mesh_stats.txt"].decode().splitlines()] == [l.split()[0] for l in single["chamfer.txt"].decode().splitlines()]
    for f in STATS_FILES:
        assert sharded[f] == single[f], (f, single[f], sharded[f])
    assert single["chamfer.txt"] == off["chamfer.txt"] == sharded["chamfer.txt"]
    assert not [f for f in listing if f.startswith("mesh_stats")]          # the run without the switch: the files removed above stay away
