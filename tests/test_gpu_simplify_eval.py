"""`--eval.simplify=2 --eval.mesh_stats` through eval_metrics and the dump on the synthetic data at vox_res 16: {idx}_mesh_simplified.ply
re-reads to ops.mesh_cluster_simplify's arrays, simplify.txt holds the op's counts, no original vertex is farther from the simplified
mesh than a cluster cell's diagonal, and the switch off leaves no file of it and every other byte alone.  No process is started here
(the two-rank run is tests/test_zz_simplify_two_ranks.py)."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
OURS = ("simplify.txt", "mesh_stats_simplified.txt")


def _read_ply(fname):
    """-> (float property names, vertices [V,3] float32, faces [F,3] int32) of a binary PLY of util_vis.write_ply_mesh."""
    data = open(fname, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[1] == "format binary_little_endian 1.0"
    props = [l.split()[2] for l in lines if l.startswith("property float")]
    n_v = int([l for l in lines if l.startswith("element vertex")][0].split()[2])
    n_f = int([l for l in lines if l.startswith("element face")][0].split()[2])
    vdt = np.dtype([(p, "<f4") for p in props])
    v = np.frombuffer(data, vdt, n_v, end)
    rec = np.frombuffer(data, np.dtype([("n", "u1"), ("i", "<i4", (3,))]), n_f, end + vdt.itemsize * n_v)
    assert (rec["n"] == 3).all() and end + vdt.itemsize * n_v + 13 * n_f == len(data)
    return props, np.stack([v["x"], v["y"], v["z"]], 1), rec["i"]


def _files(o):
    """{relative name: bytes} of the .txt files of the output folder and of every per-sample file under dump/."""
    out = {}
    for folder in ("", "dump"):
        d = os.path.join(o.output_path, folder)
        for f in sorted(os.listdir(d)) if os.path.isdir(d) else []:
            if os.path.isfile(os.path.join(d, f)) and (folder or f.endswith(".txt")):
                out[os.path.join(folder, f)] = open(os.path.join(d, f), "rb").read()
    return out


def _clear(o):
    for name in _files(o):
        os.remove(os.path.join(o.output_path, name))


def test_evaluation_writes_the_simplified_meshes_and_their_records(tmp_path):
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    from shapeclipper_amd import ops
    from shapeclipper_amd.model.runner import Runner
    from shapeclipper_amd.utils import options
    o = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_simplify", "--output_root=%s" % tmp_path,
                                             "--arch.enc_pretrained!", "--data.dataset=synthetic", "--eval.vox_res=16", "--eval.num_points=1000",
                                             "--tb!", "--eval.simplify=2", "--eval.mesh_stats"]), verbose=False)
    o.device, o.world_size, o.port = 0, 1, 0
    torch.manual_seed(0)
    r = Runner(o)
    r.load_dataset(o, eval_split="test")
    r.build_networks(o)
    seen = []
    dump = r.dump_visuals

    def spy(opt, var, ep, train=False):
        seen.append((var.idx.cpu().tolist(), var.level_vox.clone()))
        return dump(opt, var, ep, train=train)

    r.dump_visuals = spy
    lo, hi = o.eval.range
    S, k = o.eval.vox_res + 1, 2
    G = -(-(S - 1) // k)
    diagonal = math.sqrt(3.0) * k * (hi - lo) / (S - 1)                        # of a cluster cell, in object units
    results = {}
    for mode in ("evaluate", "evaluate_sharded"):
        seen.clear()
        _clear(o)
        value = getattr(r, mode)(o, ep=0)
        on = _files(o)
        lines = {int(l.split()[0]): l.split() for l in on["simplify.txt"].decode().splitlines()}
        stats = {int(l.split()[0]): l.split() for l in on["mesh_stats_simplified.txt"].decode().splitlines()}
        plain = {int(l.split()[0]): l.split() for l in on["mesh_stats.txt"].decode().splitlines()}
        print(on["simplify.txt"].decode(), on["mesh_stats_simplified.txt"].decode(), sep="\n")
        assert list(lines) == [int(l.split()[0]) for l in on["chamfer.txt"].decode().splitlines()] == list(stats)
        n_meshes = 0
        for ids, level in seen:
            packed = ops.isosurface_mesh(level)
            res = ops.mesh_cluster_simplify(*packed, (0.0, 0.0, 0.0), float(k), G, 0.05)
            world = (res.verts / S * (hi - lo) + lo).cpu().numpy()
            v_end, f_end = np.cumsum(res.v_count.numpy()), np.cumsum(res.f_count.numpy())
            for b, i in enumerate(ids):
                nv, nf = int(res.v_count[b]), int(res.f_count[b])
                f = lines[i]
                assert len(f) == 10 and len(stats[i]) == 19
                assert [int(x) for x in f[1:8]] == [k, int(packed[2][b]), nv, int(packed[3][b]), nf, int(res.collapsed[b]), int(res.cancelled[b])]
                assert int(f[4]) == nf + int(f[6]) + int(f[7])                 # marching cubes writes no degenerate face
                name = os.path.join("dump", "%d_mesh_simplified.ply" % i)
                if nf == 0:
                    assert name not in on and f[8] == f[9] == "nan"
                    continue
                props, pv, pf = _read_ply(os.path.join(o.output_path, name))
                assert props == ["x", "y", "z"]                                  # positions and faces, nothing else
                assert np.array_equal(pv.view(np.uint32), world[v_end[b] - nv:v_end[b]].view(np.uint32))
                assert np.array_equal(pf, res.faces[f_end[b] - nf:f_end[b]].cpu().numpy())
                print("sample %d: dist_mean %s dist_max %s, cell diagonal %.8f" % (i, f[8], f[9], diagonal))
                assert 0.0 <= float(f[8]) <= float(f[9]) <= diagonal
                assert int(stats[i][2]) == nf and int(stats[i][1]) + int(stats[i][9]) == nv      # faces; referenced + unreferenced vertices
                assert int(plain[i][2]) == int(f[4])
                n_meshes += 1
        assert n_meshes >= 1, mode
        # the switch off: no file of it, every other file and the returned value unchanged
        _clear(o)
        del o.eval.simplify
        assert getattr(r, mode)(o, ep=0) == value
        off = _files(o)
        o.eval.simplify = k
        assert not [f for f in off if "simplif" in f]
        assert off == {f: data for f, data in on.items() if "simplif" not in f}
        assert "chamfer.txt" in off and any(f.endswith("_mesh.ply") for f in off)
        results[mode] = on
    assert results["evaluate"].keys() == results["evaluate_sharded"].keys()
    for f in OURS:
        assert results["evaluate"][f] == results["evaluate_sharded"][f], f
    # vis_{ep}/ of the training-time visualisation: the vis_only pass decimates too and dump_geometry writes the same file
    from shapeclipper_amd.utils import eval_3D
    from shapeclipper_amd.utils.util import EasyDict as edict
    r.dump_visuals = dump
    r.graph.eval()
    o.H, o.W = o.eval.image_size
    os.makedirs(os.path.join(o.output_path, "vis_3"), exist_ok=True)
    sample = r.test_data[0]
    batch = {key: ({kk: vv[None] for kk, vv in v.items()} if isinstance(v, dict) else torch.as_tensor(v)[None]) for key, v in sample.items()}
    with torch.no_grad():
        var = r.evaluate_batch(o, edict(batch), 0, 0, single_gpu=True)
        eval_3D.eval_metrics(o, var, r.graph.module.sdf_network, vis_only=True)
        assert "mesh_simplified" in var and "mesh_stats_simplified" in var
        r.dump_geometry(o, var, "vis_3")
    name = "%d_mesh_simplified.ply" % int(var.idx[0])
    assert open(os.path.join(o.output_path, "vis_3", name), "rb").read() == results["evaluate_sharded"][os.path.join("dump", name)]       # one sample at a time there too


def test_too_many_cells_names_the_switch():
    from shapeclipper_amd.utils import eval_3D
    from shapeclipper_amd.utils.util import EasyDict as edict
    var = edict(level_vox=torch.zeros(1, 259, 1, 1, device="cuda:0"))          # only the shape is read before the refusal
    with pytest.raises(ValueError, match="eval.simplify"):
        eval_3D.meshes_simplified(edict(eval=dict(range=[-0.6, 0.6], simplify=2)), var)
