"""ops.emd_match (csrc/emd3d.hip) on the GPU against the numpy restatement tests/emd_ref.py, bit for bit on all six outputs, against the
exact optimum of scipy's linear_sum_assignment through epsilon-complementary slackness, and the evaluation's `--eval.emd` on the
pix3d_mini tree (the two-rank run of evaluate.py is in tests/test_zz_emd_two_ranks.py: tests that start other processes run behind the
kernel tests).

Shapes: n = 2 (the smallest), 64 (one wave of objects), 100 (no multiple of the wave), 192, 256 (one trip of the four-object scan), 300
(a second, partly empty trip: added to the issue's list) and 2048 (the LDS budget, run once).  The restatement of every case is computed
once per module and shared."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emd_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEV = torch.device("cuda:0")
NAMES = ("assignment", "cost", "price", "emd", "rounds", "converged")
DTYPES = (torch.int32, torch.float32, torch.float32, torch.float64, torch.int32, torch.int32)
EPS = 1e-4


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def _match(a, b, **kw):
    from shapeclipper_amd import ops
    return ops.emd_match(_dev(a), _dev(b), **kw)


def _same(got, want, what):
    """Every output of `got` (EmdResult of tensors) has the dtype of the interface and the bits of `want` (EmdRef of numpy arrays);
    torch.equal on the integer view, so NaN matches NaN of the same bits."""
    for name, dtype, g, w in zip(NAMES, DTYPES, got, want):
        w = torch.as_tensor(np.ascontiguousarray(w))
        g = g.detach().cpu()
        assert g.dtype == dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        bits = {torch.float32: torch.int32, torch.float64: torch.int64}.get(dtype, dtype)
        if not torch.equal(g.view(bits), w.view(bits)):
            bad = (g.view(bits) != w.view(bits)).nonzero()
            raise AssertionError("%s %s: %d of %d differ, first at %s: got %r, want %r" % (
                what, name, len(bad), g.numel(), bad[0].tolist(), g[tuple(bad[0])].item(), w[tuple(bad[0])].item()))


def _inputs():
    """{name: (a [B,n,3], b [B,n,3])}: the four inputs of the host test, n = 100, n = 2, n = 300, and a batch of three different clouds."""
    one = lambda p: (p[0][None], p[1][None])
    cs = {"sphere_cube_64": one(ref.sphere_cube(64)), "sphere_cube_256": one(ref.sphere_cube(256)), "lattice_64": one(ref.lattice_reverse()),
          "permuted_192": one(ref.permuted_noise(192)), "sphere_cube_100": one(ref.sphere_cube(100)), "random_2": one(ref.random_pair(2)),
          "random_300": one(ref.random_pair(300))}
    trio = [ref.sphere_cube(128, seed=3), ref.permuted_noise(128, seed=4), ref.random_pair(128, seed=5)]     # they end in different rounds
    cs["batch3_128"] = (np.stack([t[0] for t in trio]), np.stack([t[1] for t in trio]))
    return cs


@pytest.fixture(scope="module")
def cases():
    return {k: (c, ref.emd_match(*c)) for k, c in _inputs().items()}


def _check_bounds(a, b, assignment, price, emd, what):
    """Epsilon-complementary slackness in float64 and the optimum bracket, for one image; prints the figures before it asserts."""
    n = a.shape[0]
    assert sorted(assignment.tolist()) == list(range(n)), what
    c = ref.cost_matrix(a, b)
    delta = ref.slack_delta(c, price)
    excess = ref.slackness_excess(a, b, assignment, price)
    exact, _ = ref.exact_emd(a, b)
    print("%s: slackness %.6e (eps + delta = %.6e), emd - optimum %.3e" % (what, excess, EPS + delta, emd - exact))
    assert excess <= EPS + delta, what
    assert exact <= emd <= exact + EPS + delta, what


# ---- 1. bits against the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere_cube_64", "sphere_cube_256", "lattice_64", "permuted_192", "sphere_cube_100", "random_2",
                                  "random_300", "batch3_128"])
def test_bits_against_the_restatement(cases, name):
    (a, b), want = cases[name]
    got = _match(a, b)
    print(name, "rounds", got.rounds.tolist(), "emd", got.emd.tolist())
    assert bool((torch.as_tensor(want.converged) == 1).all())
    _same(got, want, name)
    if name == "batch3_128":
        assert len(set(want.rounds.tolist())) == 3          # the images of the batch do end in different rounds


def test_same_bits_on_a_second_stream_and_on_a_repeat(cases):
    (a, b), want = cases["batch3_128"]
    a, b = _dev(a), _dev(b)
    from shapeclipper_amd import ops
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = ops.emd_match(a, b)
    side.synchronize()
    _same(on_side, want, "side stream")
    _same(ops.emd_match(a, b), want, "repeat")
    for k in range(3):                                      # an image alone has the bits it has in the batch
        _same(ops.emd_match(a[k:k + 1].contiguous(), b[k:k + 1].contiguous()), type(want)(*(w[k:k + 1] for w in want)), "image %d alone" % k)


# ---- 2. the slackness and optimum bounds on the GPU outputs, independent of the restatement ------------------------------------------
@pytest.mark.parametrize("name", ["sphere_cube_64", "sphere_cube_256", "lattice_64", "permuted_192"])
def test_slackness_and_optimum_bounds(name):
    a, b = _inputs()[name]
    got = _match(a, b)
    assert got.converged.tolist() == [1]
    _check_bounds(a[0], b[0], got.assignment[0].cpu().numpy(), got.price[0].cpu().numpy(), float(got.emd[0]), name)
    cost = ref.cost_matrix(a[0], b[0])[np.arange(a.shape[1]), got.assignment[0].cpu().numpy()]
    assert torch.equal(got.cost[0].cpu(), torch.as_tensor(cost))


# ---- 3. max_rounds ends the auction and the matching is completed in index order ------------------------------------------------------
def test_max_rounds_completes_the_bijection():
    a, b = ref.sphere_cube(64)
    want = ref.emd_match(a[None], b[None], max_rounds=5)
    got = _match(a[None], b[None], max_rounds=5)
    assert got.converged.tolist() == [0] and got.rounds.tolist() == [5]
    assert sorted(got.assignment[0].tolist()) == list(range(64))
    _same(got, want, "max_rounds = 5")


# ---- 4. a NaN in one image -------------------------------------------------------------------------------------------------------------
def test_a_nan_coordinate_is_confined_to_its_image(cases):
    (a, b), want = cases["batch3_128"]
    clean = _match(a, b)
    a = a.copy()
    a[1, 17, 2] = np.nan
    got = _match(a, b)
    n = a.shape[1]
    assert got.assignment[1].tolist() == list(range(n)) and int(got.rounds[1]) == 0 and int(got.converged[1]) == 0
    assert bool(torch.isnan(got.emd[1])) and not bool(got.cost[1].any()) and not bool(got.price[1].any())
    for k in (0, 2):
        for name, g, w in zip(NAMES, got, clean):
            assert torch.equal(g[k], w[k]), (k, name)
    _same(got, ref.emd_match(a, b), "NaN in image 1")
    b2 = b.copy()
    b2[0, 0, 0] = np.inf                                    # an infinite OBJECT coordinate likewise
    got = _match(a, b2)
    assert bool(torch.isnan(got.emd[:2]).all()) and torch.equal(got.emd[2], clean.emd[2]) and got.rounds.tolist()[:2] == [0, 0]


# ---- 5. n = 2048: the LDS budget -------------------------------------------------------------------------------------------------------
def test_n_2048_converges_within_the_bounds():
    a, b = ref.random_pair(2048, seed=7)
    got = _match(a[None], b[None])
    torch.cuda.synchronize()
    print("n = 2048: rounds %d, emd %.8f" % (int(got.rounds[0]), float(got.emd[0])))
    assert got.converged.tolist() == [1]
    _check_bounds(a, b, got.assignment[0].cpu().numpy(), got.price[0].cpu().numpy(), float(got.emd[0]), "random 2048")
    # beyond what the bounds ask: the vectorised restatement takes about a second here (17,234 rounds), so the bits are compared too
    _same(got, ref.emd_match(a[None], b[None]), "random 2048")


# ---- 6. refusals that need the device ---------------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    from shapeclipper_amd import ops
    x = torch.zeros(2, 8, 3, device=DEV)
    with pytest.raises(ValueError):
        ops.emd_match(x.transpose(0, 1).contiguous().transpose(0, 1), x)          # not contiguous
    with pytest.raises(RuntimeError):
        ops.emd_match(x, x.cpu())
    empty = ops.emd_match(x[:0], x[:0])
    assert empty.assignment.shape == (0, 8) and empty.emd.shape == (0,)
    same = ops.emd_match(x, x)                              # coincident points: every cost is zero, every w ties
    assert same.converged.tolist() == [1, 1] and same.emd.tolist() == [0.0, 0.0]
    assert all(sorted(r) == list(range(8)) for r in same.assignment.tolist())


# ---- 7. the evaluation: --eval.emd on the pix3d_mini tree --------------------------------------------------------------------------------
EMD_FILES = ("emd.txt", "emd_cat.txt")
ICP_FILES = ("emd_icp.txt", "emd_cat_icp.txt")
NEW_KEYS = ("emd", "emd_n", "emd_rounds", "emd_converged", "emd_assignment")
TREE_ARGS = ["--arch.enc_pretrained!", "--tb!", "--batch_size=2", "--data.pix3d.cat=chair,sofa", "--data.num_classes=2", "--data.num_workers=0",
             "--data.max_img_cat=2", "--eval.vox_res=16", "--eval.num_points=1000"]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from shapeclipper_amd.data import pix3d_mini
    root = str(tmp_path_factory.mktemp("pix3d_emd") / "Pix3D")
    pix3d_mini.write_tree(root, n_per_cat=6, k_nearest=5, cat_key="chair,sofa", n_points=2000, seed=11)
    return root


def _opt(tree, output_root, extra=()):
    from shapeclipper_amd.utils import options
    o = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_emd", "--output_root=%s" % output_root,
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


def _by_hand(var, pred, points):
    """ops.emd_match on the documented sub-samples: the first n rows of the prediction, the rows floor(k M / n) of the ground truth."""
    from shapeclipper_amd import ops
    gt = var.dpc.points
    n = min(points, pred.shape[1], gt.shape[1])
    rows = torch.tensor([k * gt.shape[1] // n for k in range(n)], device=DEV)
    return ops.emd_match(pred[:, :n].contiguous(), gt[:, rows].contiguous(), eps=EPS), n


def test_evaluation_writes_the_emd_files_beside_the_raw_ones(tree, tmp_path, monkeypatch):
    from shapeclipper_amd.utils import eval_3D
    o = _opt(tree, str(tmp_path))
    assert "emd" not in o.eval and "emd_points" not in o.eval
    r = _runner(o)
    grid = _box_grid(o)
    monkeypatch.setattr(eval_3D, "HAVE_MESHING", False)
    monkeypatch.setattr(eval_3D, "compute_level_grid", lambda opt, net, z, pts: grid[None].repeat(pts.shape[0], 1, 1, 1))
    n_samples = len(r.test_data)
    assert n_samples == 4
    net = r.graph.module.sdf_network
    ply = ["dump/%d_pointclouds_emd.ply" % i for i in range(n_samples)]

    # ---- off: without the key, and with the key set to false: the same bytes, nothing new ----
    raw_value = r.evaluate(o, ep=0)
    off = _files(o)
    assert {"chamfer.txt", "cd_cat.txt", "f_score.txt", "dump/0_pointclouds_comp.ply"} <= set(off)
    assert not [f for f in off if "emd" in f]
    o.eval.emd, o.eval.emd_points = False, 128
    assert r.evaluate(o, ep=0) == raw_value and _files(o) == off
    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net)
    assert not [k for k in var if "emd" in k]
    raw = (var.cd_acc.clone(), var.cd_comp.clone(), var.f_score.clone(), var.dpc_pred.clone(), var.dpc.points.clone())

    # ---- on ----
    o.eval.emd = True
    assert r.evaluate(o, ep=0) == raw_value                             # the returned value is the raw one
    on = _files(o)
    for f, data in off.items():
        assert on[f] == data, f                                         # every existing output keeps its bytes
    assert sorted(set(on) - set(off)) == sorted(EMD_FILES + tuple(ply))
    lines = on["emd.txt"].decode().splitlines()
    assert len(lines) == n_samples and [int(l.split()[0]) for l in lines] == list(range(n_samples))
    labels = []
    for it, line in enumerate(lines):
        var = _sample_var(r, o, it)
        eval_3D.eval_metrics(o, var, net)
        labels.append(int(var.category_label[0]))
        assert all(k in var for k in NEW_KEYS) and "emd_icp" not in var
        res, n = _by_hand(var, var.dpc_pred, 128)
        assert n == 128 == var.emd_n and var.emd.dtype == torch.float64 and var.emd.shape == (1,) and var.emd_assignment.shape == (1, 128)
        assert torch.equal(var.emd, res.emd) and torch.equal(var.emd_assignment, res.assignment) and torch.equal(var.emd_rounds, res.rounds)
        assert line == "%d %d %.8f %d %d" % (it, n, float(res.emd[0]), int(res.rounds[0]), int(res.converged[0])), (line, res)
        assert int(res.converged[0]) == 1 and len(line.split()[2].split(".")[1]) == 8
        print("emd.txt:", line, "  chamfer.txt:", on["chamfer.txt"].decode().splitlines()[it])
        # the matching costs no less than letting every point choose its own neighbour: emd >= the accuracy over the same n points
        assert float(res.emd[0]) >= float(torch.cdist(var.dpc_pred[0, :n], var.dpc.points[0]).min(dim=1).values.double().mean()) - 1e-6
        header = on[ply[it]][:400].decode("latin1")
        assert "element vertex %d" % (2 * n) in header
    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net)
    for a, b in zip(raw, (var.cd_acc, var.cd_comp, var.f_score, var.dpc_pred, var.dpc.points)):
        assert torch.equal(a, b)                                        # the raw metrics are computed exactly as before
    cat, cat_raw = on["emd_cat.txt"].decode().splitlines(), on["cd_cat.txt"].decode().splitlines()
    assert cat[0] == "EMD    Count Cat" and len(cat) == len(cat_raw) == 3
    emds = [float(l.split()[2]) for l in lines]
    for row, row_raw in zip(cat[1:], cat_raw[1:]):
        assert row.split()[1:] == row_raw.split()[3:] and len(row.split()[0].split(".")[1]) == 4
    for c, row in enumerate(cat[1:]):                                   # cd_cat.txt's mean: the sum over the category / (count + 0.001)
        mine = [e for e, lab in zip(emds, labels) if lab == c]
        assert int(row.split()[1]) == len(mine) > 0
        assert abs(float(row.split()[0]) - sum(mine) / (len(mine) + 0.001)) <= 0.5e-4 + 1e-7       # %.4f of it, from %.8f values

    # ---- the sharded evaluation writes the same lines from its extra gather ----
    for f in EMD_FILES:
        os.remove(os.path.join(o.output_path, f))
    assert r.evaluate_sharded(o, ep=0) == pytest.approx(raw_value, rel=1e-5)
    sharded = _files(o)
    assert set(sharded) == set(on)
    assert all(sharded[f] == on[f] for f in EMD_FILES + tuple(ply))

    # ---- with --eval.icp: the _icp files, from the first n rows of the aligned prediction ----
    for f in on:                                                        # (an evaluation leaves the files of earlier ones where they are)
        if "emd" in f:
            os.remove(os.path.join(o.output_path, f))
    o.eval.emd, o.eval.icp = False, True
    assert r.evaluate(o, ep=0) == raw_value
    icp_only = _files(o)
    assert not [f for f in icp_only if "emd" in f]
    o.eval.emd = True
    assert r.evaluate(o, ep=0) == raw_value
    both = _files(o)
    for f, data in icp_only.items():
        assert both[f] == data, f
    assert sorted(set(both) - set(icp_only)) == sorted(EMD_FILES + ICP_FILES + tuple(ply)) and all(both[f] == on[f] for f in EMD_FILES)
    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net)
    res, n = _by_hand(var, var.dpc_pred_icp, 128)
    assert torch.equal(var.emd_icp, res.emd) and torch.equal(var.emd_assignment_icp, res.assignment)
    assert both["emd_icp.txt"].decode().splitlines()[0] == "0 %d %.8f %d %d" % (n, float(res.emd[0]), int(res.rounds[0]), int(res.converged[0]))
    assert both["emd_cat_icp.txt"].decode().splitlines()[0] == "EMD    Count Cat"
    for f in EMD_FILES + ICP_FILES:
        os.remove(os.path.join(o.output_path, f))
    r.evaluate_sharded(o, ep=0)
    sharded = _files(o)
    assert set(sharded) == set(both) and all(sharded[f] == both[f] for f in EMD_FILES + ICP_FILES)

    # ---- emd_points above the clouds: n = min(points, N, M) ----
    o.eval.icp, o.eval.emd_points = False, 2048
    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net)
    assert var.emd_n == 1000 and var.emd_assignment.shape == (1, 1000) and int(var.emd_converged[0]) == 1
    assert torch.equal(var.emd, _by_hand(var, var.dpc_pred, 2048)[0].emd)

    # ---- an empty mesh is n coincident points, like any cloud ----
    o.eval.emd_points = 128
    monkeypatch.setattr(eval_3D, "compute_level_grid", lambda opt, net, z, pts: torch.ones_like(grid)[None].repeat(pts.shape[0], 1, 1, 1))
    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net)
    assert int(var.emd_converged[0]) == 1 and sorted(var.emd_assignment[0].tolist()) == list(range(128))
    assert bool((var.dpc_pred[0, :128] == var.dpc_pred[0, :1]).all())
    sub_gt = var.dpc.points[0, torch.arange(128, device=DEV) * var.dpc.points.shape[1] // 128]
    want = (var.dpc_pred[0, :1] - sub_gt).norm(dim=1).double().mean()
    assert float(var.emd[0]) == pytest.approx(float(want), rel=1e-6)                        # every matching costs the same

    # ---- vis_only skips it ----
    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net, vis_only=True)
    assert not [k for k in var if "emd" in k]
