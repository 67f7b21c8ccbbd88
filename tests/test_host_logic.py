"""Host-side logic that needs no GPU: options/EasyDict semantics, weight packing, TBL layout helpers,
camera algebra and loss terms of the product vs the oracle, batch schema, checkpoint ABI."""
import copy
import math

import numpy as np
import pytest
import torch

from oracle import reference_ops as R
from shapeclipper_amd import packing, synthetic
from shapeclipper_amd.utils import camera, options
from shapeclipper_amd.utils.util import EasyDict as edict


def _opt(extra=()):
    return options.set(options.parse_arguments(["--yaml=options/pix3d/config.yaml", "--name=pytest",
                                                "--output_root=/tmp/sc_pytest"] + list(extra)), verbose=False)


def test_options_cli_semantics():
    o = _opt(["--eval.vox_res=100", "--tb!", "--resume", "--optim.lr=3.e-4", "--data.pix3d.cat=table"])
    assert o.eval.vox_res == 100 and o.tb is False and o.resume is True and o.optim.lr == 3e-4
    assert o.data.pix3d.cat == "table" and o.batch_size == 12 and o.render.rand_sample == 512
    assert (o.H, o.W) == (224, 224) and o.output_path == "/tmp/sc_pytest/pix3d_output/pytest"
    assert o.hip.deterministic_conv is False
    with pytest.raises(AssertionError):
        options.parse_arguments(["--a.b=1", "--a.b=2"])          # duplicate key
    with pytest.raises(AssertionError):
        options.parse_arguments(["a=1"])                          # must start with --
    c = copy.deepcopy(o)                                          # Loss(opt) deep-copies the options
    c.arch.impl_sdf.n_channels = 3
    assert o.arch.impl_sdf.n_channels == 64 and isinstance(c.arch, edict)


def test_reference_yaml_keys_are_all_present():
    import yaml
    keys = {"group", "name", "load", "batch_size", "max_epoch", "yaml", "seed", "gpu", "cpu", "output_root", "image_size",
            "resume", "pretrain", "pre", "arch", "eval", "data", "render", "reg", "loss_weight", "optim", "camera", "tb", "freq"}
    cfg = yaml.safe_load(open("options/pix3d/config.yaml"))
    assert keys <= set(cfg)
    assert set(cfg["loss_weight"]) == {"eikonal", "render", "mask", "normal", "nearest_img", "nearest_mask",
                                       "nearest_normal", "cam_uniform", "cam_margin", "category_reg", "cam_sym"}
    assert cfg["render"] == dict(sampler="uniform", n_samples_uniform=64, rand_sample=512, ray_uniform_fac=5, normal_model="volume")


def test_pe_slot_order_is_a_permutation_with_pads():
    cols = [packing.pe_slot_col(c) for c in range(48)]
    real = sorted(c for c in cols if c >= 0)
    assert real == list(range(39)) and cols.count(-1) == 9
    # the 13 slots that depend on coordinate c are exactly packed columns 16c..16c+15
    for c in range(3):
        for col in range(16 * c, 16 * c + 16):
            r = cols[col]
            assert r < 0 or r == c or (r - 3) % 3 == c


def test_pack_sdf_reproduces_the_reference_mlp(golden):
    g = golden("g2_networks")
    W = {k[len("pert.sdf."):]: torch.tensor(g[k]) for k in g.files if k.startswith("pert.sdf.")}
    z, pts = torch.tensor(g["z_sdf"]), torch.tensor(g["pts"])
    pack, cb = packing.pack_sdf(W, z)
    assert pack.numel() == packing.SDF_PACK_FLOATS and cb.shape == (2, 5, 64)
    xs = pts.clone(); xs[:, 0] = xs[:, 0].abs()
    e = torch.cat([R.posenc(xs, 6), torch.zeros(len(pts), 1)], 1)[:, packing._SLOT_IDX]
    o = packing.SDF_OFF
    m = lambda key, r, c: pack[o[key]:o[key] + r * c].view(r, c)
    sp = lambda a: torch.nn.functional.softplus(a, beta=100)
    img = torch.arange(256) // 128
    h = sp(e @ m("W0", 64, 48).t() + cb[img, 0])
    h = sp(torch.cat([h, e], 1) @ m("W1", 64, 112).t() + cb[img, 1])
    h = sp(torch.cat([h, e], 1) @ m("W2", 64, 112).t() + cb[img, 2])
    h = sp(h @ m("W3", 64, 64).t() + cb[img, 3])
    h = sp(h @ m("W4", 64, 64).t() + cb[img, 4])
    out = h @ m("W5", 65, 64).t() + pack[o["B5"]:o["B5"] + 65]
    assert (out[:, :1] - torch.tensor(g["sdf"])).abs().max() < 1e-5
    assert (out[:, 1:] - torch.tensor(g["feat"])).abs().max() < 1e-5


def test_pack_rgb_reproduces_the_reference_mlp(golden):
    g = golden("g2_networks")
    W = {k[len("pert.rgb."):]: torch.tensor(g[k]) for k in g.files if k.startswith("pert.rgb.")}
    z, pts, feat = torch.tensor(g["z_rgb"]), torch.tensor(g["pts"]), torch.tensor(g["feat"])
    pack, db = packing.pack_rgb(W, z)
    xs = pts.clone(); xs[:, 0] = xs[:, 0].abs()
    e = torch.cat([R.posenc(xs, 6), torch.zeros(len(pts), 1)], 1)[:, packing._SLOT_IDX]
    o = packing.RGB_OFF
    img = torch.arange(256) // 128
    r = torch.relu(torch.cat([e, feat], 1) @ pack[o["V0"]:o["V0"] + 64 * 112].view(64, 112).t() + db[img, 0])
    r = torch.relu(r @ pack[o["V1"]:o["V1"] + 4096].view(64, 64).t() + db[img, 1])
    r = torch.relu(r @ pack[o["V2"]:o["V2"] + 4096].view(64, 64).t() + db[img, 2])
    c = torch.sigmoid(r @ pack[o["V3"]:o["V3"] + 192].view(3, 64).t() + pack[o["B3"]:o["B3"] + 3])
    assert (c - torch.tensor(g["rgb"])).abs().max() < 1e-5


def test_packing_is_differentiable_to_every_original_parameter():
    cfg = R.Cfg()
    W = {k: v.requires_grad_(True) for k, v in R.init_sdf_weights(cfg, 0).items()}
    z = torch.randn(3, 64, requires_grad=True)
    pack, cb = packing.pack_sdf(W, z)
    (pack.sum() + cb.sum()).backward()
    assert all(v.grad is not None for v in W.values()) and z.grad is not None
    # latent columns receive gradient only through cbias, PE/hidden columns only through the pack
    assert torch.all(W["lin0.weight"].grad[:, :39] == 1) and torch.allclose(W["lin1.weight"].grad[:, :64], torch.full((64, 64), 1 / math.sqrt(2)))


@pytest.mark.parametrize("n", [1, 15, 16, 17, 100])
def test_tbl_roundtrip(n):
    x = torch.randn(n, 64)
    t = packing.rows_to_tbl(x)
    assert t.numel() == packing.n_tiles(n) * 1024
    assert torch.equal(packing.tbl_to_rows(t, n), x)
    # element (point p, channel c) lives at float4 block [tile][c//4][p%16], lane c%4
    p, c = n - 1, 37
    assert t.view(-1, 16, 16, 4)[p // 16, c // 4, p % 16, c % 4] == x[p, c]


def test_camera_matches_oracle_on_selected_pixels(golden):
    g = golden("g8_camera")
    o = _opt(); o.H, o.W = 8, 8
    pose, intr = torch.tensor(g["pose"]), torch.tensor(g["intr"])
    c, r = camera.get_center_and_ray(o, pose, intr=intr)
    assert torch.allclose(c, torch.tensor(g["center"]), atol=1e-6) and torch.allclose(r, torch.tensor(g["ray"]), atol=2e-6)
    idx = torch.tensor([[3, 60, 17], [0, 63, 32]])
    c2, r2 = camera.get_center_and_ray(o, pose, intr=intr, ray_idx=idx)
    assert torch.allclose(r2, torch.tensor(g["ray"]).gather(1, idx[..., None].expand(-1, -1, 3)), atol=2e-6)
    assert torch.allclose(camera.get_intr(o, torch.tensor(g["scale_focal"])), intr)
    assert torch.allclose(camera.transform_normal(torch.tensor(g["normals"]), pose), torch.tensor(g["normals_transformed"]), atol=1e-6)
    M = torch.randn(5, 3, 3) + 3 * torch.eye(3)
    assert torch.allclose(camera.inverse3x3(M) @ M, torch.eye(3).expand(5, 3, 3), atol=1e-5)
    from shapeclipper_amd.model.graph import rotation_from_trig
    Rm = rotation_from_trig(torch.tensor(g["trig_azim"]), torch.tensor(g["trig_elev"]), torch.tensor(g["trig_theta"]))
    assert torch.allclose(Rm, pose[..., :3], atol=1e-6)


def test_product_losses_match_golden(golden):
    from shapeclipper_amd.model.loss import Loss
    g = golden("g7_losses")
    o = _opt()
    L = Loss(o)
    t = lambda k: torch.tensor(g[k])
    val = lambda k: float(g["val." + k])
    assert abs(L.MSE_loss(t("pred3"), t("tgt3")).item() - val("mse")) < 1e-6
    assert abs(L.MSE_loss(t("pred3"), t("tgt3"), tolerance=0.2).item() - val("mse_tol")) < 1e-6
    assert abs(L.MSE_loss(t("eik"), 1).item() - val("mse_eik")) < 1e-6
    assert abs(L.L1_loss(t("pred3"), t("tgt3")).item() - val("l1")) < 1e-6
    assert abs(L.iou_loss(t("pm"), t("tm")).item() - val("iou")) < 1e-6
    assert abs(L.iou_loss(t("pm").clone(), t("tm"), tolerance=0.1).item() - val("iou_tol")) < 1e-6
    assert abs(L.mask_loss(t("pm"), t("tm")).item() - val("mask")) < 1e-6
    assert abs(L.normal_loss(t("npred"), t("ngt"), t("nmask"), tolerance=0.2).item() - val("normal")) < 1e-5
    assert abs(L.normal_loss(t("npred"), t("ngt"), t("nmask")).item() - val("normal_notol")) < 1e-5
    assert abs(L.cam_uniform_loss(o, t("trig")).item() - val("cam_uniform")) < 1e-6
    assert abs(L.cam_margin(o, t("trig_e"), [-90 + 1e-3, 90 - 1e-3]).item() - val("cam_margin")) < 1e-5


def test_synthetic_batch_schema_and_graph_abi():
    o = _opt(["--arch.enc_pretrained!"])
    b = synthetic.make_batch(o, 2)
    assert b.rgb_input_map.shape == (2, 3, 224, 224) and b.ray_idx.shape == (2, 512) and b.ray_idx.dtype == torch.int64
    assert b.rgb_input.shape == (2, 512, 3) and b.mask_input.shape == (2, 512, 1) and b.normal_input.shape == (2, 512, 3)
    assert b.rgb_input_NN.shape == (2, 512, 3, 5) and b.rgb_input_map_NN.shape == (2, 3, 224, 224, 5)
    assert b.ray_idx_NN.shape == (2, 512, 5) and b.pose_gt_NN.shape == (2, 3, 4, 5) and b.pose_gt.shape == (2, 3, 4)
    assert torch.equal(b.rgb_input[0, 5], b.rgb_input_map[0, :, b.ray_idx[0, 5] // 224, b.ray_idx[0, 5] % 224])
    from shapeclipper_amd.model.graph import Graph
    graph = Graph(o)
    assert [n for n, _ in graph.named_children()] == ["estimator", "sdf_network", "rgb_network", "renderer", "encoder",
                                                      "latent_proj_shape", "latent_proj_rgb", "loss_fns"]
    sd = graph.state_dict()
    for k in ("sdf_network.lin0.weight", "renderer.sdf_network.lin5.bias", "renderer.density.beta", "rgb_network.lin3.weight",
              "encoder.layer4.2.bn2.running_var", "estimator.feature_extractor.layer1.0.conv1.weight", "estimator.extr_fc.bias",
              "latent_proj_shape.0.linear1.weight", "latent_proj_rgb.2.bias"):
        assert k in sd, k
    assert abs(sum(p.numel() for p in graph.parameters()) / 1e6 - 36.8) < 0.05
    assert graph.sdf_network.lin0.weight.shape == (64, 103) and graph.sdf_network.lin1.weight.shape == (64, 167)
    assert graph.rgb_network.lin0.weight.shape == (64, 167) and graph.sdf_network.lin5.weight.shape == (65, 64)
    # same RNG stream as the reference's SDFNetwork init (oracle reproduces it, golden pins the oracle)
    from shapeclipper_amd.model.implicit import SDFNetwork
    torch.manual_seed(0)
    net = SDFNetwork(o)
    W0 = R.init_sdf_weights(R.Cfg(), 0)
    assert all(torch.equal(net.state_dict()[k], v) for k, v in W0.items())


def test_uniform_sampler_consumes_the_reference_rng_stream(golden):
    from shapeclipper_amd.model.renderer import UniformSampler
    g = golden("g6_render_train")
    o = _opt()
    torch.manual_seed(78)
    z, z_eik = UniformSampler(o).get_z_vals(o, torch.zeros(64, 3), torch.tensor(g["scale_dist"]), training=True)
    zr, zer = R.get_z_vals(R.Cfg(), 64, torch.tensor(g["scale_dist"]), True, torch.tensor(g["t_rand"]), torch.tensor(g["eik_idx"]))
    assert torch.allclose(z, zr, atol=1e-6) and torch.allclose(z_eik, zer, atol=1e-6)
    assert torch.equal(torch.empty(64, 3).uniform_(-1, 1), torch.tensor(g["eik_pts"]))    # third draw of the stream


def test_isosurface_restatement_on_a_sphere():
    """oracle/isosurface_ref.py (the checker of csrc/isosurface.hip): closed surface of the right area, on the sphere."""
    import numpy as np
    from oracle.isosurface_ref import marching_tets, triangle_areas
    S, r = 17, 0.6
    ax = np.linspace(-1, 1, S)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    tris = marching_tets((np.sqrt(X * X + Y * Y + Z * Z) - r).astype(np.float32))
    h = 2.0 / (S - 1)
    assert abs(triangle_areas(tris).sum() * h * h / (4 * np.pi * r * r) - 1) < 0.02
    p = tris.reshape(-1, 3) * h - 1
    assert np.abs(np.linalg.norm(p, axis=1) - r).max() < h * h
    # watertight: every edge of the soup is shared by exactly two triangles
    from collections import Counter
    edges = Counter()
    for t in tris:
        for a, b in ((0, 1), (1, 2), (2, 0)):
            edges[tuple(sorted((tuple(t[a]), tuple(t[b]))))] += 1
    assert set(edges.values()) == {2}


def test_importance_ray_sampler_and_its_consumer():
    """utils.util.compute_sampling_prob (reference utils/util.py:237-248, called from data/pix3d.py:236): the boundary
    distance is vigra's boundaryDistanceTransform (third party, absent here: parity unpinned) = Euclidean distance to the
    nearest pixel of the other label minus 0.5; checked against a brute force, then through the synthetic loader."""
    from shapeclipper_amd.utils import util
    o = _opt(["--arch.enc_pretrained!"])
    H = W = 24
    o.H, o.W = H, W
    o.render.rand_sample = 40
    yy, xx = np.mgrid[0:H, 0:W]
    mask = (((yy - 11.3) ** 2 + (xx - 12.1) ** 2) < 36).astype(np.float32)
    np.random.seed(0)
    idx = util.compute_sampling_prob(o, torch.tensor(mask), uniform_fac=3)
    assert idx.shape == (40,) and len(set(idx.tolist())) == 40 and 0 <= int(idx.min()) and int(idx.max()) < H * W
    np.random.seed(0)
    assert torch.equal(idx, util.compute_sampling_prob(o, torch.tensor(mask), uniform_fac=3))     # numpy global RNG, as the reference
    # brute-force boundary distance -> the same probabilities -> the same draw
    fg = np.argwhere(mask > 0.5); bg = np.argwhere(mask <= 0.5)
    d = np.zeros((H, W))
    for y in range(H):
        for x in range(W):
            other = bg if mask[y, x] > 0.5 else fg
            d[y, x] = np.sqrt(((other - np.array([y, x])) ** 2).sum(1).min()) - 0.5
    prob = 1 / (torch.from_numpy(d.astype(np.float32)) + 3)
    prob = torch.nn.functional.normalize(prob.view(-1), dim=-1, p=1).numpy().astype(np.float64)
    np.random.seed(0)
    want = np.random.choice(H * W, 40, p=prob / prob.sum(), replace=False)
    assert np.array_equal(idx.numpy(), want)
    # consumer: the synthetic loader draws every view's rays with it; they concentrate around the silhouette
    o2 = _opt(["--arch.enc_pretrained!"])
    o2.H, o2.W = o2.image_size
    np.random.seed(1)
    b = synthetic.make_batch(o2, 2, seed=0, importance=True)
    assert b.ray_idx.shape == (2, 512) and b.ray_idx.dtype == torch.int64 and b.ray_idx_NN.shape == (2, 512, 5)
    assert torch.equal(b.rgb_input[1, 7], b.rgb_input_map[1, :, b.ray_idx[1, 7] // 224, b.ray_idx[1, 7] % 224])
    m = b.mask_input_map[0, 0].numpy()
    from scipy import ndimage
    dist = np.maximum(ndimage.distance_transform_edt(m > 0.5) + ndimage.distance_transform_edt(m <= 0.5) - 0.5, 0)
    near = dist.reshape(-1)[b.ray_idx[0].numpy()].mean()
    assert near < 0.75 * dist.mean(), (near, dist.mean())      # 1/(d+3) weighting: mean distance of the drawn rays 16 px vs 27 px uniform


def test_device_side_neighbour_choice_equals_numpy_choice():
    """Graph.select_neighbours without a device->host copy: given the uniforms np.random.choice would draw, the cdf
    search in numpy's operation order picks the same neighbour, and numpy's global stream ends at the same position."""
    from shapeclipper_amd.model.graph import choice_from_uniform
    B, K = 32, 5
    for seed in range(200):
        rng = np.random.RandomState(seed)
        iou = rng.rand(B, K).astype(np.float32)
        if seed % 7 == 0:
            iou[3] = iou[3, 0]                                             # equal probabilities
        probs = torch.nn.functional.normalize((1 - torch.tensor(iou)) ** 4, dim=-1, p=1)
        pn = probs.numpy()
        np.random.seed(seed)
        ref = np.stack([np.random.choice(K, size=(1,), replace=False, p=pn[i] / np.sum(pn[i])) for i in range(B)])[:, 0]
        next_ref = np.random.random_sample()
        np.random.seed(seed)
        u = np.random.random_sample(B)
        next_got = np.random.random_sample()
        idx, nan = choice_from_uniform(probs, torch.from_numpy(u))
        assert np.array_equal(idx.numpy(), ref) and next_got == next_ref and not bool(nan)
    _, nan = choice_from_uniform(torch.zeros(2, 5), torch.rand(2).double())       # all neighbours identical to the input: 0/0
    assert bool(nan)


def test_bench_self_launch_builds_the_launcher_command(monkeypatch):
    """`python bench.py --gpus N` with no launcher environment re-executes itself under torch.distributed.run exactly as the driver's N > 1
    command does (VERDICT r04 next #1a): one rank per GPU on one node, rendezvous on 127.0.0.1, every argument passed through; fewer visible
    devices than ranks is refused unless the gloo test backend is selected.  No GPU needed: the launch itself is intercepted."""
    import importlib.util
    import os
    import subprocess
    import sys
    import types
    import torch
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    spec = importlib.util.spec_from_file_location("sc_bench_for_launch_test", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    seen = {}
    monkeypatch.setattr(subprocess, "call", lambda cmd, env=None: seen.update(cmd=cmd, env=env) or 0)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--steps", "7", "--opt=--hip.reserve_cus=16"])
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 8)
    monkeypatch.delenv("SC_BENCH_BACKEND", raising=False)
    assert bench.self_launch(types.SimpleNamespace(gpus=8)) == 0
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"] and "--nnodes=1" in cmd
    assert cmd[cmd.index("--nproc-per-node") + 1] == "8" and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert int(cmd[cmd.index("--master-port") + 1]) > 0
    assert cmd[-5:] == ["--gpus", "8", "--steps", "7", "--opt=--hip.reserve_cus=16"] and cmd[-6].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    with pytest.raises(SystemExit) as e:
        bench.self_launch(types.SimpleNamespace(gpus=8))
    assert "one rank per device" in str(e.value)
    monkeypatch.setenv("SC_BENCH_BACKEND", "gloo")
    assert bench.self_launch(types.SimpleNamespace(gpus=8)) == 0


def _load_bench():
    import importlib.util
    import os
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    spec = importlib.util.spec_from_file_location("sc_bench_for_report_test", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


RAW_ENTRY_POINTS = ["sc_sdf_forward", "sc_sdf_forward_stream", "sc_sdf_backward", "sc_sdf_backward_fused", "sc_rgb_composite_forward", "sc_rgb_composite_forward_stash",
                    "sc_rgb_composite_forward_split",
                    "sc_rgb_composite_backward", "sc_rgb_composite_backward_v3", "sc_rgb_composite_backward_fused",
                    "sc_rgb_composite_backward_fused_stash", "sc_rgb_composite_backward_fused_split"]


@pytest.mark.parametrize("dominant", RAW_ENTRY_POINTS)
@pytest.mark.parametrize("batch", [1, 32])
def test_bench_timing_report_with_every_entry_point_dominant(dominant, batch):
    """VERDICT r05 #1b: the round-5 bench line died with KeyError when a RENAMED entry point (`sc_rgb_composite_backward_fused_stash` ->
    `sc_rgb_composite_backward`) was the largest entry of the timed region (8 ranks x 1 image sharing a GPU).  Feed the extraction a
    synthetic timing dict in which every raw entry point dominates in turn: it must return a roofline for the STABLE name, with the
    arithmetic of the line (achieved = FLOPs per point x points / mean of the 2 x steps largest launches), and limiter / traffic that
    belong to that kernel and no other."""
    bench = _load_bench()
    steps, rays = 3, 512
    durations = {n: [0.05, 0.04] * steps + [0.001] * (2 * steps) for n in RAW_ENTRY_POINTS if n != dominant}
    durations[dominant] = [2.0, 1.0] * steps + [0.03] * (2 * steps)              # two main renders per step + two eikonal launches
    durations["sc_wgrad"] = [0.2] * (6 * steps)
    durations["sc_loss_fused_forward"] = [5.0] * steps                          # larger than everything, but not a scored kernel
    durations["sc_never_launched"] = []
    n_pts = batch * rays * 64
    per, roof, roof_w = bench.timing_report(durations, steps, n_pts, batch)
    stable = bench.STABLE_NAME.get(dominant, dominant)
    assert "error" not in roof and roof["kernel"] == stable
    assert set(per) == {bench.STABLE_NAME.get(n, n) for n in durations if durations[n]}
    assert roof["launch_ms"] == pytest.approx(1.5) and roof["points_per_launch"] == n_pts
    want = bench.FLOPS_PER_POINT[stable] * n_pts / 1.5e-3 / 1e12
    assert roof["achieved"] == pytest.approx(want, abs=0.006) and roof["frac"] == pytest.approx(want / 157.3, abs=1e-4)
    assert roof["limiter"] == bench.LIMITER[stable]
    if batch == 32:            # committed PMC constant of THIS kernel (profiles/rNN_traffic.json), or null when it has none
        import json
        import os
        root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
        known = {}
        for prof in ("r01", "r02", "r03", "r04", "r05", "r06"):
            f = os.path.join(root, "profiles", prof + "_traffic.json")
            if os.path.exists(f):
                for k, v in json.load(open(f))["kernels"].items():
                    known[k] = v["traffic_bytes"]
        assert roof["traffic"] == known.get(stable)
    else:
        assert roof["traffic"] is None and roof["bound"] == "mfma"
    # merged entries: the calls of every raw name that maps to one stable name add up
    merged_calls = sum(len(d) for n, d in durations.items() if bench.STABLE_NAME.get(n, n) == stable)
    assert per[stable]["calls"] == merged_calls
    assert roof_w is not None and roof_w["frac"] > 0


def test_bench_timing_report_degenerate_inputs():
    bench = _load_bench()
    per, roof, roof_w = bench.timing_report({}, 2, 1024, 1)
    assert per == {} and "error" in roof and roof_w is None
    per, roof, roof_w = bench.timing_report({"sc_loss_fused_forward": [1.0]}, 2, 1024, 1)
    assert "error" in roof and "sc_loss_fused_forward" in per
    # fewer launches than 2 x steps (a rank that rendered once): the mean is over what there is
    per, roof, _ = bench.timing_report({"sc_rgb_composite_backward_fused_stash": [1.0]}, 4, 1024, 1)
    assert roof["kernel"] == "sc_rgb_composite_backward" and roof["launch_ms"] == 1.0
    assert bench._guarded(lambda: 1 / 0)["error"].startswith("ZeroDivisionError")


def test_bench_dump_outputs_writes_the_step_and_samples_at_fixed_positions(tmp_path, monkeypatch):
    """`bench.py --dump-outputs DIR`: losses (float64), what the forward wrote into the batch dict (not its inputs), weights, buffers and
    gradients (float32; large tensors sampled at positions fixed by the name); --steps below 1 is refused."""
    import sys
    bench = _load_bench()
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(3, 3000), torch.nn.BatchNorm1d(3000))
    x = torch.randn(4, 3)
    inputs = edict(rgb_input=x, idx=torch.arange(4))
    var = edict(inputs)
    var.rgb_recon = net(x)
    loss = edict(render=var.rgb_recon.square().mean())
    loss.all = 2 * loss.render
    loss.all.backward()

    def dump(d):
        info = bench.dump_outputs(str(d), loss, var, inputs, net)
        return info, {f.name: np.load(f) for f in d.iterdir()}
    info, got = dump(tmp_path / "a")
    assert info["files"] == len(got) and info["bytes"] == sum(a.nbytes for a in got.values()) <= bench.DUMP_LIMIT_BYTES
    assert {"loss.all.npy", "loss.render.npy", "var.rgb_recon.npy", "param.0.weight.npy", "param.1.running_mean.npy",
            "param.1.num_batches_tracked.npy", "grad.0.weight.npy", "grad.1.bias.npy"} <= set(got)
    assert not any(n.startswith(("var.rgb_input", "var.idx")) for n in got)
    assert got["loss.all.npy"].dtype == np.float64 and got["loss.all.npy"] == np.float64(loss.all.item())
    assert all(a.dtype == np.float32 for n, a in got.items() if not n.startswith("loss."))
    assert np.array_equal(got["var.rgb_recon.npy"], var.rgb_recon.detach().numpy().ravel())           # 12000 elements: kept whole
    w = net[0].weight.detach().numpy().ravel()
    assert got["param.0.weight.npy"].shape == (bench.DUMP_SAMPLE,) and np.isin(got["param.0.weight.npy"], w).all()
    _, again = dump(tmp_path / "b")
    assert all(np.array_equal(got[n], again[n]) for n in got)                                          # same positions every run
    for argv in (["bench.py", "--steps", "3"], ["bench.py", "--steps", "0"]):
        monkeypatch.setattr(sys, "argv", argv)
        if argv[-1] == "0":
            with pytest.raises(SystemExit):
                bench.parse()
        else:
            assert bench.parse().steps == 3 and bench.parse().dump_outputs is None


def test_bench_plain_and_full_options(monkeypatch):
    """A plain `bench.py` run times no extra steps; `--full` turns the secondary measurements on with their defaults, and an option that
    asks for one of them without `--full` is refused instead of being dropped."""
    import sys
    bench = _load_bench()

    def parse(*args):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + list(args))
        return bench.parse()
    a = parse("--gpus", "1", "--steps", "5", "--warmup", "2")
    assert not a.full and a.sustained == 0
    a = parse("--full")
    assert a.full and a.sustained == 200 and a.alt_steps == 60 and a.cpu_batch == 0
    a = parse("--full", "--sustained", "0", "--alt-steps", "3", "--cpu-batch", "4")
    assert a.sustained == 0 and a.alt_steps == 3 and a.cpu_batch == 4
    a = parse("--sustained", "0", "--no-alt", "--no-cpu-baseline", "--no-workloads")        # switching extras off is harmless
    assert not a.full and a.sustained == 0
    assert parse("--workloads-only", "--with-reference-gpu").with_reference_gpu
    for extra in (["--sustained", "2"], ["--alt-steps", "3"], ["--cpu-batch", "4"], ["--with-reference-gpu"]):
        with pytest.raises(SystemExit):
            parse(*extra)


def test_gpu_suite_runs_parity_tests_before_subprocess_tests():
    """VERDICT r05 #1c: the driver runs `pytest -m gpu -x`; a timing-dependent subprocess test must never stand in front of a kernel-vs-oracle
    test.  Every test_gpu_*.py file is placed by tests/conftest.py::suite_order_key; files that launch other processes sort last."""
    import glob
    import os
    import re
    from conftest import suite_order_key, _FIRST, _LAST
    here = os.path.dirname(os.path.abspath(__file__))
    files = sorted(os.path.basename(f) for f in glob.glob(os.path.join(here, "test_gpu_*.py")))
    assert set(_FIRST) | set(_LAST) <= set(files), sorted((set(_FIRST) | set(_LAST)) - set(files))
    ordered = sorted(files, key=suite_order_key)
    assert ordered[-1] == "test_gpu_bench_contract.py" and ordered[0] == "test_gpu_sdf.py"
    launches = re.compile(r"subprocess\.(run|Popen|call)|multiprocessing|mp\.spawn|torch\.distributed\.run")
    first_launcher = min(i for i, f in enumerate(ordered) if launches.search(open(os.path.join(here, f)).read()))
    for f in ordered[first_launcher:]:
        assert suite_order_key(f)[0] == 2, "%s runs after a subprocess test but is not in the last group" % f
    for f in ordered[:first_launcher]:
        assert not launches.search(open(os.path.join(here, f)).read())


# ---- the hip.* switch table (utils/options.py) and the render-path choice (ops.py) ---------------------------------------------------------
def test_hip_defaults_are_the_35_known_switches():
    assert options.HIP_DEFAULTS == dict(hip=dict(
        device_rng=False, device_choice=True, device_rays=True, device_clip_preprocess=True, fused_backward=True, deterministic_conv=False,
        fused_loss=True, fused_adam=True, guarded_step=True, batched_encoders=True, two_streams=True, overlap_allreduce=False, reserve_cus=0,
        fused_block=True, fused_bottleneck=True, fused_rgb_wgrad=True, rgb_stash=True, value_split=True, rgb_split=True, rgb_bwd_split=True,
        sdf_stream=True, upload_stream=True, rocblas=True, conv3x3=True, conv3x3_split=True, conv_stem=True, conv1x1=True, conv3x3s2=True,
        conv3x3s2_grads=True, train_vis=False, mesh_color=False, largest_component=False, surface_render=False, surface_refine=3,
        surface_scale=1))
    assert len(options.HIP_DEFAULTS["hip"]) == 35 == len(options.HIP_TABLE)
    assert list(options.HIP_DEFAULTS["hip"]) == [row.key for row in options.HIP_TABLE]
    for row in options.HIP_TABLE:
        assert row.text and (row.kind is bool) == isinstance(row.default, bool), row.key
    assert options.HIP["surface_refine"].kind == (0, 16) and options.HIP["surface_scale"].kind == (1, 4)


def test_hip_accessor_answers_with_the_table_default_and_refuses_unknown_keys():
    for row in options.HIP_TABLE:
        assert options.hip(edict(), row.key) == row.default and type(options.hip(edict(), row.key)) is type(row.default)
        assert options.hip(edict(hip=edict()), row.key) == row.default
    o = edict(hip=edict(fused_loss=False, surface_refine=7))
    assert options.hip(o, "fused_loss") is False and options.hip(o, "surface_refine") == 7 and options.hip(o, "fused_adam") is True
    for tree in (edict(), o, _opt()):
        with pytest.raises(KeyError):
            options.hip(tree, "no_such")
    assert _opt(["--hip.no_such=3"]).hip.no_such == 3            # an unknown flag on the command line is tolerated, as before


def test_each_switch_drives_exactly_its_module_attribute():
    import importlib
    driven = {row.key: row.drives for row in options.HIP_TABLE if row.drives is not None}
    assert driven == dict(
        fused_block=("model.resnet", "FUSED_BLOCK"), fused_bottleneck=("model.view_estimator", "HIP_BOTTLENECK"),
        fused_rgb_wgrad=("ops", "FUSED_RGB_WGRAD"), rgb_stash=("ops", "RGB_STASH"), value_split=("ops", "SDF_VALUE_SPLIT"),
        rgb_split=("ops", "RGB_FWD_SPLIT"), rgb_bwd_split=("ops", "RGB_BWD_SPLIT"), sdf_stream=("ops", "SDF_FWD_STREAM"),
        upload_stream=("model.renderer", "UPLOAD_STREAM"), conv3x3=("model.resnet", "HIP_CONV3X3"),
        conv3x3_split=("model.resnet", "HIP_CONV3X3_SPLIT"), conv_stem=("model.resnet", "HIP_CONV_STEM"),
        conv1x1=("model.resnet", "HIP_CONV_1X1"), conv3x3s2=("model.resnet", "HIP_CONV3X3_S2"),
        conv3x3s2_grads=("model.resnet", "HIP_CONV3X3_S2_GRADS"))
    read = lambda: {d: getattr(importlib.import_module("shapeclipper_amd." + d[0]), d[1]) for d in driven.values()}
    try:
        _opt()
        base = read()
        assert base == {d: True for d in driven.values()}
        for key, target in driven.items():
            assert options.HIP[key].default is True
            _opt(["--hip.%s!" % key])
            want = dict(base)
            want[target] = False
            if key in ("rgb_stash", "fused_rgb_wgrad"):         # the one derived rule: the split reverse chain needs both
                want[("ops", "RGB_BWD_SPLIT")] = False
            assert read() == want, key
            _opt(["--hip.%s" % key])                             # stated explicitly: the default again
            assert read() == base, key
            _opt(["--hip.%s!" % key])
            _opt()                                               # a default set restores every attribute
            assert read() == base, key
    finally:
        _opt()
    assert options.HIP_REQUIRES == {"rgb_bwd_split": ("rgb_stash", "fused_rgb_wgrad")}


def test_render_entry_points_follow_the_switches(monkeypatch):
    """ops.sdf_forward_entry / rgb_reverse_form / rgb_forward_parks against tables written out from the inline conditions they replaced:
    sdf_forward took the value chain for SDF_VALUE_SPLIT and not (want_grad or want_feat or stash), the streamed kernel for SDF_FWD_STREAM
    and want_grad and (not stash or want_feat), else sc_sdf_forward; rgb_composite_backward took the fused family for FUSED_RGB_WGRAD and
    n_images <= 256 (_split / _stash with parked activations by RGB_BWD_SPLIT), else _v3; the forward parked for RGB_STASH and
    FUSED_RGB_WGRAD and n_images <= 256."""
    import itertools
    from shapeclipper_amd import ops
    tf = (False, True)
    V, S, P = "sc_sdf_value_forward_split", "sc_sdf_forward_stream", "sc_sdf_forward"
    sdf_want = {     # (SDF_VALUE_SPLIT, SDF_FWD_STREAM) -> (want_grad, want_feat, stash) = FFF FFT FTF FTT TFF TFT TTF TTT
        (True, True): (V, P, P, P, S, P, S, S),
        (True, False): (V, P, P, P, P, P, P, P),
        (False, True): (P, P, P, P, S, P, S, S),
        (False, False): (P, P, P, P, P, P, P, P)}
    for (vs, st), row in sdf_want.items():
        monkeypatch.setattr(ops, "SDF_VALUE_SPLIT", vs)
        monkeypatch.setattr(ops, "SDF_FWD_STREAM", st)
        for args, want in zip(itertools.product(tf, tf, tf), row):
            assert ops.sdf_forward_entry(*args) == want, (vs, st, args)
    stem = "sc_rgb_composite_backward_"
    v3, fu, sp, sh = stem + "v3", stem + "fused", stem + "fused_split", stem + "fused_stash"
    rgb_want = {     # (FUSED_RGB_WGRAD, RGB_BWD_SPLIT) -> (n_images, parked) = (1,F) (1,T) (256,F) (256,T) (257,F) (257,T); RGB_STASH: no part
        (True, True): (fu, sp, fu, sp, v3, v3),
        (True, False): (fu, sh, fu, sh, v3, v3),
        (False, True): (v3, v3, v3, v3, v3, v3),
        (False, False): (v3, v3, v3, v3, v3, v3)}
    parks_want = {   # (RGB_STASH, FUSED_RGB_WGRAD) -> n_images = 1, 256, 257; RGB_BWD_SPLIT: no part
        (True, True): (True, True, False), (True, False): (False, False, False),
        (False, True): (False, False, False), (False, False): (False, False, False)}
    for stash, fused, bwd in itertools.product(tf, tf, tf):
        monkeypatch.setattr(ops, "RGB_STASH", stash)
        monkeypatch.setattr(ops, "FUSED_RGB_WGRAD", fused)
        monkeypatch.setattr(ops, "RGB_BWD_SPLIT", bwd)
        for (n, parked), want in zip(itertools.product((1, 256, 257), tf), rgb_want[fused, bwd]):
            assert ops.rgb_reverse_form(n, parked) == want, (stash, fused, bwd, n, parked)
        for n, want in zip((1, 256, 257), parks_want[stash, fused]):
            assert ops.rgb_forward_parks(n) is want, (stash, fused, bwd, n)
