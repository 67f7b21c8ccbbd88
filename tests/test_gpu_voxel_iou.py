"""ops.voxel_frame / voxel_solid / voxel_iou (csrc/voxel_solid.hip) on the GPU against the numpy restatement tests/voxel_iou_ref.py, every
output on the integer view, and the evaluation's `--eval.iou` on the pix3d_mini tree (the two-rank run of evaluate.py is in
tests/test_zz_iou_two_ranks.py: tests that start other processes run behind the kernel tests).

Shapes: N = 1, N = 100 (no multiple of the wave), coincident points, R = 8 with close = 2 (the smallest interior: indices 3..4), R = 33
(an odd grid, words partly used), R = 64 (full words, 96 KiB of LDS) at close 0, 1 and 2, N = 100,000 once, a serpentine channel that
the exterior walks in hundreds of sweeps, rows that are not finite, and a batch of three pairs.  The restatement of every case is computed
once per module and shared."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_iou_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEV = torch.device("cuda:0")
F = np.float32
BITS = {torch.float32: torch.int32, torch.float64: torch.int64}


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def _same(got, want, what):
    """The tensor `got` has the dtype, the shape and the bits of the numpy array `want` (NaN matches NaN of the same bits)."""
    w = torch.as_tensor(np.ascontiguousarray(want))
    g = got.detach().cpu()
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    view = BITS.get(g.dtype, g.dtype)
    if not torch.equal(g.view(view), w.view(view)):
        bad = (g.view(view) != w.view(view)).nonzero()
        raise AssertionError("%s: %d of %d differ, first at %s: got %r, want %r" % (
            what, len(bad), g.numel(), bad[0].tolist(), g[tuple(bad[0])].item(), w[tuple(bad[0])].item()))


def _gpu_pair(a, b, res, close):
    """The whole chain on the device: frame of the pair, the two solids, the popcounts."""
    from shapeclipper_amd import ops
    a, b = _dev(a), _dev(b)
    origin, pitch = ops.voxel_frame(a, b, res, close)
    sa, sb = ops.voxel_solid(a, origin, pitch, res, close), ops.voxel_solid(b, origin, pitch, res, close)
    inter, union = ops.voxel_iou(sa.bits, sb.bits)
    return dict(origin=origin, pitch=pitch, inter=inter, union=union, **{"a_" + k: v for k, v in sa._asdict().items()},
                **{"b_" + k: v for k, v in sb._asdict().items()})


def _ref_pair(a, b, res, close):
    origin, pitch = ref.voxel_frame(a, b, res, close)
    sa, sb = ref.voxel_solid(a, origin, pitch, res, close), ref.voxel_solid(b, origin, pitch, res, close)
    inter, union = ref.voxel_iou(sa.bits, sb.bits)
    return dict(origin=origin, pitch=pitch, inter=inter, union=union, **{"a_" + k: v for k, v in sa._asdict().items()},
                **{"b_" + k: v for k, v in sb._asdict().items()})


def _compare(got, want, what):
    assert sorted(got) == sorted(want)
    for k in want:
        _same(got[k], want[k], "%s %s" % (what, k))


def _inputs():
    """{name: (a [B,N,3], b [B,M,3], res, close)}."""
    one = lambda p: (p[0][None], p[1][None])
    rng = np.random.RandomState(3)
    cs = {"n_1": (*one((rng.uniform(-1, 1, (1, 3)).astype(F), rng.uniform(-1, 1, (1, 3)).astype(F))), 32, 1),
          "n_100": (*one(ref.shape_pair("sphere", n=100)), 32, 1),
          "coincident": (np.full((1, 50, 3), 0.25, F), np.full((1, 70, 3), 0.25, F), 32, 1),
          "r8_close2": (*one(ref.shape_pair("box", n=2000)), 8, 2),
          "r33": (*one(ref.shape_pair("chair", n=5000)), 33, 1),
          "r32_close0": (*one(ref.shape_pair("chair", n=20000)), 32, 0),
          "r32_close2": (*one(ref.shape_pair("chair", n=20000)), 32, 2),
          "r64_close0": (*one(ref.shape_pair("torus", n=20000)), 64, 0),
          "r64_close1": (*one(ref.shape_pair("torus", n=20000)), 64, 1),
          "r64_close2": (*one(ref.shape_pair("torus", n=20000)), 64, 2),
          "n_100000": (ref.sphere(100000, seed=2)[None], ref.box_surface(90001, half=(0.45, 0.4, 0.3), seed=3)[None], 64, 1)}
    trio = [ref.shape_pair(name, n=3000, seed=7 + k) for k, name in enumerate(("sphere", "chair", "torus"))]
    cs["batch3"] = (np.stack([t[0] for t in trio]), np.stack([t[1] for t in trio]), 32, 1)
    return cs


@pytest.fixture(scope="module")
def cases():
    return {k: (c, _ref_pair(*c)) for k, c in _inputs().items()}


# ---- 1. bits against the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n_1", "n_100", "coincident", "r8_close2", "r33", "r32_close0", "r32_close2", "r64_close0", "r64_close1",
                                  "r64_close2", "n_100000", "batch3"])
def test_bits_against_the_restatement(cases, name):
    (a, b, res, close), want = cases[name]
    got = _gpu_pair(a, b, res, close)
    print(name, "shell", got["a_shell_voxels"].tolist(), got["b_shell_voxels"].tolist(), "solid", got["a_solid_voxels"].tolist(),
          got["b_solid_voxels"].tolist(), "sweeps", got["a_sweeps"].tolist(), got["b_sweeps"].tolist(), "inter", got["inter"].tolist(),
          "union", got["union"].tolist())
    _compare(got, want, name)
    assert got["a_bits"].shape == (a.shape[0], res, res)
    if name == "coincident":
        assert got["pitch"].tolist() == [1.0] and got["inter"].tolist() == [1] and got["union"].tolist() == [1]
    if name == "r8_close2":
        assert int(want["a_solid_voxels"][0]) <= 8                      # indices 3..4 on every axis
    if name == "r64_close1":
        assert int(want["a_solid_voxels"][0]) > 3 * int(want["a_shell_voxels"][0])   # closed, the torus fills


@pytest.mark.parametrize("res", [32, 64])
def test_serpentine_channel(res):
    """The exterior walks the corridors one voxel a sweep: 408 sweeps at R = 32, 1,832 at R = 64 (the restatement's counts)."""
    from shapeclipper_amd import ops
    pts, origin, pitch = ref.serpentine(res)
    want = ref.voxel_solid(pts[None], origin[None], np.array([pitch], F), res, 0)
    got = ops.voxel_solid(_dev(pts[None]), _dev(origin[None]), _dev(np.array([pitch], F)), res, 0)
    print("serpentine R = %d: %d points, %d sweeps" % (res, len(pts), int(got.sweeps[0])))
    assert int(want.sweeps[0]) > 300 and int(want.solid_voxels[0]) == int(want.shell_voxels[0]) == len(pts)
    for k in want._fields:
        _same(getattr(got, k), getattr(want, k), "serpentine %s" % k)


def test_rows_that_are_not_finite(cases):
    """In a given frame a NaN or Inf row sets nothing; the frame of a pair with such a row is NaN, the solids are empty, and the other
    images of the batch keep their bits."""
    from shapeclipper_amd import ops
    (a, b, res, close), want = cases["batch3"]
    dirty = a.copy()
    dirty[1, 5] = [np.nan, 0.0, 0.0]
    dirty[1, 9] = [0.0, np.inf, 0.0]
    dirty[1, 2999] = [0.0, 0.0, -np.inf]
    got = ops.voxel_solid(_dev(dirty), _dev(want["origin"]), _dev(want["pitch"]), res, close)
    ref_dirty = ref.voxel_solid(dirty, want["origin"], want["pitch"], res, close)
    for k in ref_dirty._fields:
        _same(getattr(got, k), getattr(ref_dirty, k), "dirty rows, clean frame: %s" % k)
    for k in (0, 2):
        assert torch.equal(got.bits[k].cpu(), torch.as_tensor(want["a_bits"][k]))
    pair = _gpu_pair(dirty, b, res, close)
    _compare(pair, _ref_pair(dirty, b, res, close), "dirty rows, own frame")
    assert bool(torch.isnan(pair["origin"][1]).all()) and bool(torch.isnan(pair["pitch"][1]))
    assert pair["a_solid_voxels"].tolist()[1] == 0 and pair["b_solid_voxels"].tolist()[1] == 0 and pair["union"].tolist()[1] == 0
    for k in (0, 2):
        assert torch.equal(pair["a_bits"][k].cpu(), torch.as_tensor(want["a_bits"][k])) and int(pair["inter"][k]) == int(want["inter"][k])


def test_a_batch_is_its_images_and_runs_repeat(cases):
    (a, b, res, close), want = cases["batch3"]
    assert len({int(v) for v in want["a_solid_voxels"]}) == 3
    for k in range(3):                                      # an image alone has the bits it has in the batch
        _compare(_gpu_pair(a[k:k + 1], b[k:k + 1], res, close), {n: v[k:k + 1] for n, v in want.items()}, "image %d alone" % k)
    _compare(_gpu_pair(a, b, res, close), want, "repeat")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = _gpu_pair(a, b, res, close)
    side.synchronize()
    _compare(on_side, want, "side stream")


def test_voxel_iou_against_numpy_popcounts():
    from shapeclipper_amd import ops
    rng = np.random.RandomState(0)
    a = rng.randint(-2 ** 63, 2 ** 63, (4, 33, 33), dtype=np.int64)
    b = rng.randint(-2 ** 63, 2 ** 63, (4, 33, 33), dtype=np.int64)
    a[2] = b[2] = 0                                         # an empty union
    a[3] = b[3] = -1                                        # every bit
    inter, union = ops.voxel_iou(_dev(a), _dev(b))
    want_i, want_u = ref.voxel_iou(a, b)
    _same(inter, want_i, "inter")
    _same(union, want_u, "union")
    assert inter.tolist()[2:] == [0, 64 * 33 * 33] and union.tolist()[2:] == [0, 64 * 33 * 33]
    flat = ops.voxel_iou(_dev(a.reshape(4, -1)), _dev(b.reshape(4, -1)))
    assert torch.equal(flat[0], inter) and torch.equal(flat[1], union)


def test_refusals_on_the_device():
    from shapeclipper_amd import ops
    x, o, p = torch.zeros(2, 8, 3, device=DEV), torch.zeros(2, 3, device=DEV), torch.ones(2, device=DEV)
    with pytest.raises(ValueError):
        ops.voxel_frame(x.transpose(0, 1).contiguous().transpose(0, 1), x)            # not contiguous
    with pytest.raises(RuntimeError):
        ops.voxel_solid(x, o.cpu(), p)
    empty = ops.voxel_solid(x[:0], o[:0], p[:0], 16, 0)
    assert empty.bits.shape == (0, 16, 16) and empty.sweeps.shape == (0,)
    assert ops.voxel_frame(x[:0], x[:0])[0].shape == (0, 3)
    bad = ops.voxel_solid(x, o, torch.tensor([0.0, -1.0], device=DEV), 16, 0)         # pitch <= 0: nothing is set
    assert bad.shell_voxels.tolist() == [0, 0] and bad.solid_voxels.tolist() == [0, 0] and not bool(bad.bits.any())


# ---- 2. the evaluation: --eval.iou on the pix3d_mini tree --------------------------------------------------------------------------------
IOU_FILES = ("iou.txt", "iou_cat.txt")
ICP_FILES = ("iou_icp.txt", "iou_cat_icp.txt")
TREE_ARGS = ["--arch.enc_pretrained!", "--tb!", "--batch_size=2", "--data.pix3d.cat=chair,sofa", "--data.num_classes=2", "--data.num_workers=0",
             "--data.max_img_cat=2", "--eval.vox_res=16", "--eval.num_points=1000"]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from shapeclipper_amd.data import pix3d_mini
    root = str(tmp_path_factory.mktemp("pix3d_iou") / "Pix3D")
    pix3d_mini.write_tree(root, n_per_cat=6, k_nearest=5, cat_key="chair,sofa", n_points=2000, seed=11)
    return root


def _opt(tree, output_root, extra=()):
    from shapeclipper_amd.utils import options
    o = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_iou", "--output_root=%s" % output_root,
                                             "--data.pix3d.root=%s" % tree, *TREE_ARGS, *extra]), verbose=False)
    o.device, o.world_size, o.port = 0, 1, 0
    return o


def _runner(o):
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    from shapeclipper_amd.model.runner import Runner
    torch.manual_seed(0)
    r = Runner(o)
    r.load_dataset(o, eval_split="test")
    r.build_networks(o)
    r.graph.eval()
    return r


def _box_grid(o):
    """A level grid whose solid is the box |x| < .3, |y| < .2, |z| < .25, at get_dense_3D_grid's positions."""
    lo, hi = o.eval.range
    g = torch.linspace(lo, hi, o.eval.vox_res + 1, device=DEV)
    pts = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), dim=-1)
    return (pts.abs() - torch.tensor([0.3, 0.2, 0.25], device=DEV)).amax(dim=-1).contiguous()


def _sample_var(r, o, it=0):
    from shapeclipper_amd.utils.util import EasyDict as edict
    sample = r.test_data[it]
    batch = {k: ({kk: vv[None] for kk, vv in v.items()} if isinstance(v, dict) else torch.as_tensor(v)[None]) for k, v in sample.items()}
    o.H, o.W = o.eval.image_size
    with torch.no_grad():
        return r.evaluate_batch(o, edict(batch), 0, it, single_gpu=True)


def _files(o):
    """{relative name: bytes} of the .txt files of the output folder and of every per-sample file under dump/."""
    out = {}
    for folder in ("", "dump"):
        d = os.path.join(o.output_path, folder)
        for f in sorted(os.listdir(d)) if os.path.isdir(d) else []:
            if os.path.isfile(os.path.join(d, f)) and (folder or f.endswith(".txt")):
                out[os.path.join(folder, f)] = open(os.path.join(d, f), "rb").read()
    return out


def _line(it, res, iou, inter, union, sa, sb):
    return "%d %d %.8f %d %d %d %d %d %d" % (it, res, iou, inter, union, sa.solid_voxels, sb.solid_voxels, sa.shell_voxels, sb.shell_voxels)


def test_evaluation_writes_the_iou_files_beside_the_raw_ones(tree, tmp_path, monkeypatch):
    from shapeclipper_amd.utils import eval_3D
    o = _opt(tree, str(tmp_path))
    assert not [k for k in o.eval if "iou" in k]
    r = _runner(o)
    grid = _box_grid(o)
    monkeypatch.setattr(eval_3D, "HAVE_MESHING", False)
    monkeypatch.setattr(eval_3D, "compute_level_grid", lambda opt, net, z, pts: grid[None].repeat(pts.shape[0], 1, 1, 1))
    n_samples = len(r.test_data)
    assert n_samples == 4
    net = r.graph.module.sdf_network
    ply = ["dump/%d_voxels_comp.ply" % i for i in range(n_samples)]

    # ---- off: without the key, and with the key set to false: the same files, the same bytes ----
    raw_value = r.evaluate(o, ep=0)
    off = _files(o)
    assert {"chamfer.txt", "cd_cat.txt", "f_score.txt", "dump/0_pointclouds_comp.ply"} <= set(off)
    assert not [f for f in off if "iou" in f or "voxels" in f]
    o.eval.iou, o.eval.iou_res, o.eval.iou_close = False, 24, 2
    assert r.evaluate(o, ep=0) == raw_value and _files(o) == off
    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net)
    assert not [k for k in var if "iou" in k]
    raw = (var.cd_acc.clone(), var.cd_comp.clone(), var.f_score.clone(), var.dpc_pred.clone(), var.dpc.points.clone())

    # ---- on ----
    o.eval.iou = True
    assert r.evaluate(o, ep=0) == raw_value                             # the returned value is the raw one
    on = _files(o)
    for f, data in off.items():
        assert on[f] == data, f                                         # every existing output keeps its bytes
    assert sorted(set(on) - set(off)) == sorted(IOU_FILES + tuple(ply))
    lines = on["iou.txt"].decode().splitlines()
    assert len(lines) == n_samples and [int(l.split()[0]) for l in lines] == list(range(n_samples))
    labels, ious = [], []
    for it, line in enumerate(lines):
        var = _sample_var(r, o, it)
        eval_3D.eval_metrics(o, var, net)
        labels.append(int(var.category_label[0]))
        assert "iou_icp" not in var and var.iou_res == 24 and var.iou.dtype == torch.float64 and var.iou.shape == (1,)
        iou, inter, union, sa, sb = ref.pair_iou(var.dpc_pred[0].cpu().numpy(), var.dpc.points[0].cpu().numpy(), 24, 2)
        ious.append(iou)
        assert float(var.iou[0]) == iou == inter / union and (int(var.iou_inter[0]), int(var.iou_union[0])) == (inter, union)
        assert (int(var.iou_vox_pred[0]), int(var.iou_vox_gt[0])) == (sa.solid_voxels, sb.solid_voxels)
        assert (int(var.iou_shell_pred[0]), int(var.iou_shell_gt[0])) == (sa.shell_voxels, sb.shell_voxels)
        assert line == _line(it, 24, iou, inter, union, sa, sb), (line, iou, inter, union)
        assert len(line.split()) == 9 and len(line.split()[2].split(".")[1]) == 8
        print("iou.txt:", line, "  chamfer.txt:", on["chamfer.txt"].decode().splitlines()[it])
        assert "element vertex %d" % (sa.solid_voxels + sb.solid_voxels) in on[ply[it]][:400].decode("latin1")
        centres = eval_3D.voxel_centres(var.iou_bits_pred[0], var.iou_origin[0], var.iou_pitch[0])
        assert centres.shape == (sa.solid_voxels, 3)
        index = np.argwhere(ref.unpack(sa.bits))
        assert np.array_equal(np.floor((centres.numpy() - var.iou_origin[0].cpu().numpy()) / float(var.iou_pitch[0])).astype(np.int64), index)
    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net)
    for a, b in zip(raw, (var.cd_acc, var.cd_comp, var.f_score, var.dpc_pred, var.dpc.points)):
        assert torch.equal(a, b)                                        # the raw metrics are computed exactly as before
    cat, cat_raw = on["iou_cat.txt"].decode().splitlines(), on["cd_cat.txt"].decode().splitlines()
    assert cat[0] == "IoU    Count Cat" and len(cat) == len(cat_raw) == 3
    for row, row_raw in zip(cat[1:], cat_raw[1:]):
        assert row.split()[1:] == row_raw.split()[3:] and len(row.split()[0].split(".")[1]) == 4
    for c, row in enumerate(cat[1:]):                                   # cd_cat.txt's mean: the sum over the category / (count + 0.001)
        mine = [e for e, lab in zip(ious, labels) if lab == c]
        assert int(row.split()[1]) == len(mine) > 0
        assert abs(float(row.split()[0]) - sum(mine) / (len(mine) + 0.001)) <= 0.5e-4 + 1e-9

    # ---- the sharded evaluation writes the same lines from its extra gather ----
    for f in IOU_FILES:
        os.remove(os.path.join(o.output_path, f))
    assert r.evaluate_sharded(o, ep=0) == pytest.approx(raw_value, rel=1e-5)
    sharded = _files(o)
    assert set(sharded) == set(on)
    assert all(sharded[f] == on[f] for f in IOU_FILES + tuple(ply))

    # ---- with --eval.icp: the _icp files, in the frame of the aligned prediction and the ground truth ----
    o.eval.icp = True
    assert r.evaluate(o, ep=0) == raw_value
    both = _files(o)
    assert set(IOU_FILES + ICP_FILES + tuple(ply)) <= set(both) and all(both[f] == on[f] for f in on)
    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net)
    iou, inter, union, sa, sb = ref.pair_iou(var.dpc_pred_icp[0].cpu().numpy(), var.dpc.points[0].cpu().numpy(), 24, 2)
    assert float(var.iou_icp[0]) == iou and int(var.iou_vox_gt_icp[0]) == sb.solid_voxels
    assert both["iou_icp.txt"].decode().splitlines()[0] == _line(0, 24, iou, inter, union, sa, sb)
    assert both["iou_cat_icp.txt"].decode().splitlines()[0] == "IoU    Count Cat"

    # ---- vis_only skips it ----
    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net, vis_only=True)
    assert not [k for k in var if "iou" in k]
