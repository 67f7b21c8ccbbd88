"""Coloured meshes with vertex normals: ops.rgb_points_forward (csrc/rgb_points.hip), eval_3D.mesh_attributes and `--hip.mesh_color`.

What is pinned: the colours of the kernel against RGBNetwork.forward in float64 (oracle/reference_ops.py) and bit-level against the
rgb_flat of the render kernel at the same points; the normals against the unit float64 gradient; the tail of a partial tile (nothing
stored past n_points); that the attributes are evaluated at the level grid's sample positions, not at the written (rescaled) vertices;
the eager path of other architectures; empty level sets; Runner.evaluate / evaluate_sharded writing {idx}_mesh_color.ply without
changing any other output."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _padded(counts, rng, scale=0.6):
    """Random points of len(counts) images in the per-image layout of mesh_attributes: image b at rows [b P, b P + V_b), P = 16 ceil(max
    V_b / 16), padding rows repeating the image's first point.  -> (points [B P, 3] fp32, P, valid row mask)."""
    P = 16 * ((max(counts) + 15) // 16)
    pts = np.zeros((len(counts), P, 3), np.float32)
    valid = np.zeros((len(counts), P), bool)
    for b, v in enumerate(counts):
        pts[b, :v] = rng.uniform(-scale, scale, (v, 3))
        pts[b, v:] = pts[b, 0]
        valid[b, :v] = True
    return torch.tensor(pts.reshape(-1, 3)), P, valid.reshape(-1)


def _weights(cfg, seed):
    from oracle import reference_ops as R
    Ws, Wr = R.init_sdf_weights(cfg, seed), R.init_rgb_weights(cfg, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    for W in (Ws, Wr):
        for k in W:
            W[k] = W[k] + 0.03 * torch.randn(W[k].shape, generator=g)
    return Ws, Wr


def _reference(cfg, Ws, Wr, pts, B, zs, zr):
    """float64 colours and unit normals at pts [B P, 3] (P points per image)."""
    from oracle import reference_ops as R
    d = lambda W: {k: v.double() for k, v in W.items()}
    p = pts.double().clone()
    _, feat, grad = R.sdf_conditional(cfg, d(Ws), B, p, zs.double(), compute_grad=True)
    P = pts.shape[0] // B
    rgb = R.rgb_mlp(cfg, d(Wr), p.detach(), zr.double().repeat_interleave(P, 0), feat.detach())
    grad = grad.detach()
    return rgb.detach(), grad / grad.norm(dim=1, keepdim=True)


def _device_attributes(cfg, Ws, Wr, pts, n_per_image, zs, zr, n=None):
    from shapeclipper_amd import ops, packing
    w_pack, cbias = packing.pack_sdf(Ws, zs)
    v_pack, dbias = packing.pack_rgb(Wr, zr, n_sdf=cfg.hidden_sdf)
    q = pts[:n].to(DEV).contiguous() if n is not None else pts.to(DEV)
    _, grad, feat = ops.sdf_forward(q, w_pack.to(DEV), cbias.to(DEV), n_per_image, symmetric=cfg.force_symmetry)
    return ops.rgb_points_forward(q, grad, feat, v_pack.to(DEV), dbias.to(DEV), n_per_image, cfg.force_symmetry), (q, grad, feat, v_pack.to(DEV), dbias.to(DEV))


SMALL = dict(hidden_sdf=48, hidden_rgb=32, posenc_rgb=4)


@pytest.mark.parametrize("sym", [True, False])
@pytest.mark.parametrize("arch", ["shipped", "small"])
def test_points_against_float64(sym, arch):
    from oracle import reference_ops as R
    cfg = R.Cfg(force_symmetry=sym, **(SMALL if arch == "small" else {}))
    Ws, Wr = _weights(cfg, 3 if sym else 4)
    rng = np.random.RandomState(0)
    sizes = (1, 15, 16, 17, 1000, 65537) if arch == "shipped" else (17, 1000)
    cases = [[n] for n in sizes] + [[700, 33, 1], [5, 300, 129]]
    worst_c = worst_n = 0.0
    for counts in cases:
        B = len(counts)
        zs, zr = torch.randn(B, cfg.latent_sdf), torch.randn(B, cfg.latent_rgb)
        pts, P, valid = _padded(counts, rng)
        # the last image ends at its last vertex: the final tile of the launch is partial unless V_last % 16 == 0
        n = (B - 1) * P + counts[-1]
        (rgb, normal), _ = _device_attributes(cfg, Ws, Wr, pts, P, zs, zr, n=n)
        assert rgb.shape == normal.shape == (n, 3)
        want_c, want_n = _reference(cfg, Ws, Wr, pts, B, zs, zr)
        keep = torch.tensor(valid[:n])
        ec = (rgb.cpu().double() - want_c[:n])[keep].abs().max().item()
        en = (normal.cpu().double() - want_n[:n])[keep].abs().max().item()
        assert ec < 2e-5 and en < 2e-4, (counts, ec, en)
        worst_c, worst_n = max(worst_c, ec), max(worst_n, en)
    print("rgb_points %s sym=%s: worst colour error %.2e, worst normal error %.2e" % (arch, sym, worst_c, worst_n))


def test_nothing_is_read_or_written_past_n_points():
    """Direct C-ABI call into outputs longer than n_points (sentinels behind the end) for partial final tiles; only-rgb / only-normal
    calls; n_points = 0 and a bad n_per_image."""
    from oracle import reference_ops as R
    from shapeclipper_amd import _lib, ops
    cfg = R.Cfg()
    Ws, Wr = _weights(cfg, 7)
    lib = _lib.load()
    zs, zr = torch.randn(1, 64), torch.randn(1, 64)
    for n in (1, 15, 17, 33):
        pts = torch.tensor(np.random.RandomState(n).uniform(-0.5, 0.5, (n, 3)).astype(np.float32))
        (rgb, normal), (q, grad, feat, v_pack, dbias) = _device_attributes(cfg, Ws, Wr, pts, 48, zs, zr)
        out_c = torch.full((n + 16, 3), -7.0, device=DEV)
        out_n = torch.full((n + 16, 3), -7.0, device=DEV)
        code = lib.sc_rgb_points_forward_split(_lib.ptr(q), _lib.ptr(grad), _lib.ptr(feat), _lib.ptr(v_pack), _lib.ptr(dbias), ctypes.c_int(n),
                                               ctypes.c_int(48), ctypes.c_int(1), ctypes.c_int(1), _lib.ptr(out_c), _lib.ptr(out_n), _lib.stream())
        assert code == 0
        assert torch.equal(out_c[:n], rgb) and torch.equal(out_n[:n], normal)
        assert (out_c[n:] == -7.0).all() and (out_n[n:] == -7.0).all()
        only_c, none_n = ops.rgb_points_forward(q, grad, feat, v_pack, dbias, 48, True, want_normal=False)
        none_c, only_n = ops.rgb_points_forward(q, grad, feat, v_pack, dbias, 48, True, want_rgb=False)
        assert none_n is None and none_c is None and torch.equal(only_c, rgb) and torch.equal(only_n, normal)
    empty = torch.zeros(0, 3, device=DEV)
    c0, n0 = ops.rgb_points_forward(empty, empty, torch.zeros(0, device=DEV), v_pack, dbias, 16, True)
    assert c0.shape == n0.shape == (0, 3)
    code = lib.sc_rgb_points_forward_split(_lib.ptr(q), _lib.ptr(grad), _lib.ptr(feat), _lib.ptr(v_pack), _lib.ptr(dbias), ctypes.c_int(4),
                                           ctypes.c_int(40), ctypes.c_int(1), ctypes.c_int(1), _lib.ptr(out_c), _lib.ptr(out_n), _lib.stream())
    assert code == 1                                                                 # hipErrorInvalidValue: n_per_image % 16 != 0
    with pytest.raises(ValueError, match="multiple of 16"):
        ops.rgb_points_forward(q, grad, feat, v_pack, dbias, 40, True)


def test_colours_equal_the_render_kernels():
    """The same points laid out as rays of 64 samples: rgb_points_forward's colours against rgb_composite_forward's rgb_flat (the same
    pre-split chain: bit-identical expected)."""
    from oracle import reference_ops as R
    from shapeclipper_amd import ops, packing
    cfg = R.Cfg()
    Ws, Wr = _weights(cfg, 11)
    B, rays = 3, 40
    zs, zr = torch.randn(B, 64), torch.randn(B, 64)
    pts = torch.tensor(np.random.RandomState(2).uniform(-0.7, 0.7, (B * rays * 64, 3)).astype(np.float32)).to(DEV)
    w_pack, cbias = (t.to(DEV) for t in packing.pack_sdf(Ws, zs))
    v_pack, dbias = (t.to(DEV) for t in packing.pack_rgb(Wr, zr))
    sdf, grad, feat = ops.sdf_forward(pts, w_pack, cbias, rays * 64, symmetric=True)
    z_vals = torch.linspace(0.5, 2.5, 64, device=DEV).repeat(B * rays, 1).contiguous()
    out = ops.rgb_composite_forward(pts, z_vals, torch.ones(B * rays, device=DEV), sdf, grad, feat, v_pack, dbias,
                                    torch.tensor([0.1], device=DEV), rays, True, 1e-4, 1.0, 1.0, keep_rgb_flat=True)
    rgb, _ = ops.rgb_points_forward(pts, grad, feat, v_pack, dbias, rays * 64, True, want_normal=False)
    diff = (rgb - out["rgb_flat"]).abs().max().item()
    print("rgb_points vs rgb_flat: max |diff| %.3e, bit-identical: %s" % (diff, torch.equal(rgb, out["rgb_flat"])))
    assert diff <= 1e-6


def _opt(extra=(), output_root="/tmp/sc_pytest"):
    from shapeclipper_amd.utils import options
    return options.set(options.parse_arguments(["--yaml=options/pix3d/config.yaml", "--name=pytest_mesh_color", "--output_root=%s" % output_root,
                                                *extra]), verbose=False)


def _sphere_level(opt, sdf_net, z):
    from shapeclipper_amd.utils import eval_3D
    from shapeclipper_amd.utils.util import EasyDict as edict
    var = edict(idx=torch.zeros(z.shape[0], dtype=torch.long, device=DEV))
    return eval_3D.compute_level_grid(opt, sdf_net, z, eval_3D.get_dense_3D_grid(opt, var))


def _query_positions(opt, level):
    """The grid-sample positions of every vertex (the same expression as mesh_attributes), per image."""
    from shapeclipper_amd import ops
    lo, hi = opt.eval.range
    S = level.shape[1]
    verts, _, vc, _ = ops.isosurface_mesh(level)
    q = lo + verts * ((hi - lo) / (S - 1))
    ends = np.cumsum(vc.numpy()).tolist()
    return [q[e - int(v):e] for e, v in zip(ends, vc.tolist())]


def test_query_positions_lie_on_the_level_set():
    from shapeclipper_amd import ops
    from shapeclipper_amd.model.implicit import RGBNetwork, SDFNetwork
    from shapeclipper_amd.utils import eval_3D
    opt = _opt(["--eval.vox_res=64"])
    torch.manual_seed(0)
    sdf_net, rgb_net = SDFNetwork(opt).to(DEV), RGBNetwork(opt).to(DEV)
    z = torch.zeros(1, opt.arch.impl_sdf.proj_latent_dim, device=DEV)
    zr = torch.zeros(1, opt.arch.impl_rgb.proj_latent_dim, device=DEV)
    level = _sphere_level(opt, sdf_net, z)
    (verts, faces, normals, colours), = eval_3D.mesh_attributes(opt, sdf_net, rgb_net, z, zr, level)
    (q,) = _query_positions(opt, level)
    assert verts.shape == q.shape == normals.shape == colours.shape and verts.shape[0] > 1000 and faces.shape[1] == 3
    assert colours.dtype == torch.uint8 and normals.dtype == verts.dtype == torch.float32
    lo, hi = opt.eval.range
    assert torch.equal(verts, eval_3D.meshes_device(level, lo, hi)[0][0])          # written as {idx}_mesh.ply writes them
    w_pack, cbias = sdf_net.packed(z)
    at = lambda p: ops.sdf_forward(p.contiguous(), w_pack, cbias, p.shape[0], symmetric=True, want_grad=False, want_feat=False)[0].abs()
    s_query, s_written = at(q), at(verts)
    print("|sdf| at the query positions: max %.2e mean %.2e; at the written vertices: mean %.2e"
          % (s_query.max().item(), s_query.mean().item(), s_written.mean().item()))
    assert s_query.max().item() < 1e-3
    assert s_written.mean().item() >= 10 * s_query.mean().item()
    assert (normals.norm(dim=1) - 1).abs().max().item() < 1e-5
    # the geometric init is a lumpy sphere (random hidden layers: its zero level set lies between radius ~0.38 and ~0.62 here), so its
    # normals are not radial to 0.99 everywhere: they point outward, and they are the network's own unit gradient at the query positions
    radial = (normals * q / q.norm(dim=1, keepdim=True)).sum(dim=1)
    print("radial component of the normals: min %.3f mean %.3f" % (radial.min().item(), radial.mean().item()))
    assert radial.min().item() > 0.5 and radial.mean().item() > 0.9
    from oracle import reference_ops as R
    Ws = {k: v.detach().cpu() for k, v in sdf_net.weight_dict().items()}
    Wr = {k: v.detach().cpu() for k, v in rgb_net.weight_dict().items()}
    _, want_n = _reference(R.Cfg(), Ws, Wr, q.cpu(), 1, z.cpu(), zr.cpu())
    assert (normals.cpu().double() - want_n).abs().max().item() < 2e-4


def _check_quantised(colours, want):
    """colours uint8 = trunc(clamp(c, 0, 1) * 255) of a c within 2e-5 of want (float64)."""
    c = colours.cpu().double()
    t = want.clamp(0, 1) * 255
    assert (c <= t + 255 * 2e-5).all() and (c > t - 1 - 255 * 2e-5).all()


def test_mesh_attributes_against_float64():
    """mesh_attributes on the HIP path, two images (one of them empty) against the float64 network at the query positions."""
    from oracle import reference_ops as R
    from shapeclipper_amd.model.implicit import RGBNetwork, SDFNetwork
    from shapeclipper_amd.utils import eval_3D
    opt = _opt(["--eval.vox_res=40"])
    torch.manual_seed(1)
    sdf_net, rgb_net = SDFNetwork(opt), RGBNetwork(opt)
    with torch.no_grad():
        for p in rgb_net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    sdf_net, rgb_net = sdf_net.to(DEV), rgb_net.to(DEV)
    z = torch.zeros(2, 64, device=DEV)
    zr = torch.randn(2, 64, device=DEV)
    level = _sphere_level(opt, sdf_net, z)
    level[1] = 1.0                                                                 # no sign change: an empty mesh
    (verts, faces, normals, colours), empty = eval_3D.mesh_attributes(opt, sdf_net, rgb_net, z, zr, level)
    assert all(t.shape[0] == 0 for t in empty) and verts.shape[0] > 100
    (q,), cfg = _query_positions(opt, level[:1]), R.Cfg()
    Ws = {k: v.detach().cpu() for k, v in sdf_net.weight_dict().items()}
    Wr = {k: v.detach().cpu() for k, v in rgb_net.weight_dict().items()}
    want_c, want_n = _reference(cfg, Ws, Wr, q.cpu(), 1, z[:1].cpu(), zr[:1].cpu())
    assert (normals.cpu().double() - want_n).abs().max().item() < 2e-4
    _check_quantised(colours, want_c)


def test_eager_architecture():
    """A 6 x 128 SDF network (outside the compiled family): mesh_attributes runs on stock operators and meets the same bars."""
    from oracle import reference_ops as R
    from shapeclipper_amd.model.implicit import RGBNetwork, SDFNetwork
    from shapeclipper_amd.utils import eval_3D
    opt = _opt(["--eval.vox_res=32", "--arch.impl_sdf.n_hidden_layers=6", "--arch.impl_sdf.n_channels=128"])
    torch.manual_seed(2)
    sdf_net, rgb_net = SDFNetwork(opt), RGBNetwork(opt)
    assert sdf_net.eager and rgb_net.eager
    with torch.no_grad():                                                          # (the SDF keeps its geometric init: a sphere)
        for p in rgb_net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    sdf_net, rgb_net = sdf_net.to(DEV), rgb_net.to(DEV)
    z, zr = 0.1 * torch.randn(1, 64, device=DEV), torch.randn(1, 64, device=DEV)
    level = _sphere_level(opt, sdf_net, z)
    (verts, faces, normals, colours), = eval_3D.mesh_attributes(opt, sdf_net, rgb_net, z, zr, level)
    (q,) = _query_positions(opt, level)
    assert verts.shape[0] > 100 and normals.shape == q.shape
    cfg = R.Cfg(hidden_sdf=128, n_hidden_sdf=6)
    Ws = {k: v.detach().cpu() for k, v in sdf_net.weight_dict().items()}
    Wr = {k: v.detach().cpu() for k, v in rgb_net.weight_dict().items()}
    want_c, want_n = _reference(cfg, Ws, Wr, q.cpu(), 1, z.cpu(), zr.cpu())
    assert (normals.cpu().double() - want_n).abs().max().item() < 2e-4
    _check_quantised(colours, want_c)


def test_empty_level_set_writes_nothing(tmp_path, capsys):
    from shapeclipper_amd.model.implicit import RGBNetwork, SDFNetwork
    from shapeclipper_amd.utils import eval_3D, util_vis
    from shapeclipper_amd.utils.util import EasyDict as edict
    opt = _opt(["--eval.vox_res=16"])
    sdf_net, rgb_net = SDFNetwork(opt).to(DEV), RGBNetwork(opt).to(DEV)
    level = torch.full((2, 17, 17, 17), 0.5, device=DEV)
    out = eval_3D.mesh_attributes(opt, sdf_net, rgb_net, torch.zeros(2, 64, device=DEV), torch.zeros(2, 64, device=DEV), level)
    assert len(out) == 2 and all(t.shape[0] == 0 for o in out for t in o)
    os.makedirs(tmp_path / "dump")
    util_vis.dump_meshes(edict(output_path=str(tmp_path)), [0, 1], "mesh_color", out)
    assert os.listdir(tmp_path / "dump") == [] and capsys.readouterr().out.count("Mesh is empty!") == 2


# ---- end to end: the evaluation's dumps --------------------------------------------------------------------------------------------
def _read(fname):
    data = open(fname, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    types = {"float": "<f4", "uchar": "u1"}
    vdt = np.dtype([(l.split()[2], types[l.split()[1]]) for l in lines if l.startswith("property ") and "list" not in l])
    n_v = int(lines[2].split()[2])
    n_f = int([l for l in lines if l.startswith("element face")][0].split()[2])
    v = np.frombuffer(data, vdt, n_v, end)
    f = np.frombuffer(data, np.dtype([("n", "u1"), ("i", "<i4", (3,))]), n_f, end + vdt.itemsize * n_v)["i"]
    return v, f


def _cols(v, *names):
    return np.stack([v[n] for n in names], 1)


def test_evaluate_writes_coloured_meshes(tmp_path):
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    from shapeclipper_amd.model.runner import Runner
    from shapeclipper_amd.utils import eval_3D
    o = _opt(["--arch.enc_pretrained!", "--data.dataset=synthetic", "--eval.vox_res=16", "--eval.num_points=1000", "--tb!", "--hip.mesh_color"],
             output_root=str(tmp_path))
    o.device, o.world_size, o.port = 0, 1, 0
    torch.manual_seed(0)
    r = Runner(o)
    r.load_dataset(o, eval_split="test")
    r.build_networks(o)
    net = r.graph.module
    seen = []
    dump = r.dump_visuals

    def spy(opt, var, ep, train=False):
        seen.append((var.idx.cpu().tolist(), var.level_vox.clone(), var.proj_latent_sdf.clone(), var.proj_latent_rgb.clone()))
        return dump(opt, var, ep, train=train)

    out = os.path.join(o.output_path, "dump")
    files = lambda: {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out)) if f.endswith(".ply")}
    texts = lambda: tuple(open(os.path.join(o.output_path, f)).read() for f in ("chamfer.txt", "f_score.txt"))

    r.dump_visuals = spy
    results = {}
    for mode in ("evaluate", "evaluate_sharded"):
        seen.clear()
        for f in os.listdir(out) if os.path.isdir(out) else []:
            os.remove(os.path.join(out, f))
        o.hip.mesh_color = True
        getattr(r, mode)(o, ep=0)
        on_files, on_texts = files(), texts()
        n_coloured = 0
        for ids, level, zs, zr in seen:
            attrs = eval_3D.mesh_attributes(o, net.sdf_network, net.rgb_network, zs, zr, level)
            for (v_, f_, n_, c_), i in zip(attrs, ids):
                name = "%d_mesh_color.ply" % i
                if f_.shape[0] == 0:
                    assert name not in on_files
                    continue
                v, f = _read(os.path.join(out, name))
                pv, pf = _read(os.path.join(out, "%d_mesh.ply" % i))
                assert list(v.dtype.names) == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
                if not eval_3D.HAVE_MESHING:
                    assert np.array_equal(_cols(v, "x", "y", "z"), _cols(pv, "x", "y", "z")) and np.array_equal(f, pf)
                assert np.array_equal(_cols(v, "x", "y", "z"), v_.cpu().numpy()) and np.array_equal(f, f_.cpu().numpy())
                assert np.array_equal(_cols(v, "nx", "ny", "nz"), n_.cpu().numpy())
                assert np.array_equal(_cols(v, "red", "green", "blue"), c_.cpu().numpy())
                n_coloured += 1
        assert n_coloured >= 1, mode
        # the switch off: no coloured file, every other file and the metrics byte-identical
        for f in os.listdir(out):
            os.remove(os.path.join(out, f))
        o.hip.mesh_color = False
        getattr(r, mode)(o, ep=0)
        off_files = files()
        assert not any(f.endswith("_mesh_color.ply") for f in off_files)
        assert off_files == {k: v for k, v in on_files.items() if not k.endswith("_mesh_color.ply")}
        assert texts() == on_texts
        results[mode] = on_files
    assert results["evaluate"].keys() == results["evaluate_sharded"].keys()


def test_training_visualisation_writes_coloured_meshes(tmp_path):
    """vis_{ep}/ of Runner.dump_train_vis: the coloured mesh next to the plain one when the switch is on."""
    from shapeclipper_amd.model.runner import Runner
    from shapeclipper_amd.utils import eval_3D
    from shapeclipper_amd.utils.util import EasyDict as edict
    o = _opt(["--arch.enc_pretrained!", "--data.dataset=synthetic", "--eval.vox_res=16", "--eval.num_points=1000", "--tb!", "--hip.mesh_color"],
             output_root=str(tmp_path))
    o.device, o.world_size, o.port = 0, 1, 0
    torch.manual_seed(0)
    r = Runner(o)
    r.load_dataset(o, eval_split="test")
    r.build_networks(o)
    r.graph.eval()
    o.H, o.W = o.eval.image_size
    folder = os.path.join(o.output_path, "vis_3")
    os.makedirs(folder, exist_ok=True)
    n_coloured = 0
    for it in range(len(r.test_data)):
        sample = r.test_data[it]
        batch = {k: ({kk: vv[None] for kk, vv in v.items()} if isinstance(v, dict) else torch.as_tensor(v)[None]) for k, v in sample.items()}
        with torch.no_grad():
            var = r.evaluate_batch(o, edict(batch), 0, 0, single_gpu=True)
            eval_3D.eval_metrics(o, var, r.graph.module.sdf_network, vis_only=True)
            r.dump_geometry(o, var, "vis_3")
        i = int(var.idx[0])
        names = os.listdir(folder)
        assert ("%d_mesh.ply" % i in names) == ("%d_mesh_color.ply" % i in names)
        if "%d_mesh_color.ply" % i in names:
            v, _ = _read(os.path.join(folder, "%d_mesh_color.ply" % i))
            assert "red" in v.dtype.names and "nx" in v.dtype.names
            n_coloured += 1
    assert n_coloured >= 1
