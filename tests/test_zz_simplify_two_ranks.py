"""`evaluate.py --eval.simplify=2 --eval.mesh_stats` on the pix3d_mini tree in one process and under the launcher with two ranks.  A file of
its own, named to sort behind every kernel test: tests that start other processes must not stand in front of a kernel-against-restatement
test (tests/conftest.py orders the suite by file; tests/test_host_logic.py holds every test_gpu_*.py file outside the last group to that)."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SIMPLIFY_FILES = ("simplify.txt", "mesh_stats_simplified.txt")
TREE_ARGS = ["--arch.enc_pretrained!", "--tb!", "--batch_size=2", "--data.pix3d.cat=chair,sofa", "--data.num_classes=2", "--data.num_workers=0",
             "--data.max_img_cat=2", "--eval.vox_res=16", "--eval.num_points=1000"]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from shapeclipper_amd.data import pix3d_mini
    root = str(tmp_path_factory.mktemp("pix3d_simplify_ranks") / "Pix3D")
    pix3d_mini.write_tree(root, n_per_cat=6, k_nearest=5, cat_key="chair,sofa", n_points=2000, seed=11)
    return root


def test_two_gloo_ranks_of_evaluate_py_write_the_unsharded_lines(tree, tmp_path):
    """evaluate.py with --eval.simplify=2 --eval.mesh_stats on the pix3d_mini tree (seeded random weights, no checkpoint) in one process
    and under the launcher with two ranks on the one GPU over gloo: rank 0's extra gather gives simplify.txt and
    mesh_stats_simplified.txt of the single process, byte for byte; simplify.txt has one line of 10 fields per sample; chamfer.txt is
    that of a run without the switch, which writes no file of it."""
    import socket
    import subprocess
    args = ["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=simplify_e2e", "--output_root=%s" % tmp_path, "--data.pix3d.root=%s" % tree,
            *TREE_ARGS]
    on = ["--eval.simplify=2", "--eval.mesh_stats"]
    env = dict(os.environ, MIOPEN_LOG_LEVEL="1", MIOPEN_FIND_MODE="FAST", SHAPECLIPPER_DIST_BACKEND="gloo")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = os.path.join(str(tmp_path), "pix3d_output", "simplify_e2e")
    ours = lambda f: "simplif" in f

    def run(cmd, files):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        got = {f: open(os.path.join(out, f), "rb").read() for f in files}
        listing = sorted(os.listdir(out)) + sorted(os.listdir(os.path.join(out, "dump")))
        for folder in ("", "dump"):
            for f in os.listdir(os.path.join(out, folder)):
                if f in got or ours(f):
                    os.remove(os.path.join(out, folder, f))
        return got, listing

    single, listing_single = run([sys.executable, os.path.join(ROOT, "evaluate.py")] + args + on, SIMPLIFY_FILES + ("chamfer.txt",))
    sharded, listing_sharded = run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                                    "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "evaluate.py")] + args + on,
                                   SIMPLIFY_FILES + ("chamfer.txt",))
    off, listing = run([sys.executable, os.path.join(ROOT, "evaluate.py")] + args + ["--eval.mesh_stats"], ("chamfer.txt",))
    print(single["simplify.txt"].decode(), single["mesh_stats_simplified.txt"].decode(), sep="\n")
    lines = single["simplify.txt"].decode().splitlines()
    assert len(lines) == 4 and all(len(l.split()) == 10 and l.split()[1] == "2" for l in lines), lines
    stats = single["mesh_stats_simplified.txt"].decode().splitlines()
    assert len(stats) == 4 and all(len(l.split()) == 19 for l in stats), stats
    assert [l.split()[0] for l in lines] == [l.split()[0] for l in single["chamfer.txt"].decode().splitlines()] == [l.split()[0] for l in stats]
    for f in SIMPLIFY_FILES:
        assert sharded[f] == single[f], (f, single[f], sharded[f])
    assert single["chamfer.txt"] == off["chamfer.txt"] == sharded["chamfer.txt"]
    assert [f for f in listing_single if ours(f)] == [f for f in listing_sharded if ours(f)]       # the same PLYs from the two ranks
    for l in lines:                                                             # a PLY for every sample whose simplified mesh has a face
        assert ("%s_mesh_simplified.ply" % l.split()[0] in listing_single) == (int(l.split()[5]) > 0)
    assert not [f for f in listing if ours(f)]                                  # the run without the switch: the files removed above stay away
