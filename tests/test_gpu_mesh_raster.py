"""The triangle rasteriser: csrc/mesh_raster.hip (ops.mesh_raster), eval_3D.mesh_render and `--eval.mesh_render`.

What is pinned: face, depth, barycentrics and stats bit for bit against tests/mesh_raster_ref.py (the numpy restatement of
include/shapeclipper_hip.h) on hand-built meshes that exercise every rule and on marching-cubes meshes; that the thread path and the
wave path write the same bytes; that nothing is written outside the outputs; the partition of one-face images; the derived sphere
shells on the device mesh; determinism, batch invariance and view permutation; the refusals; eval_3D.mesh_render's colours against
ops.texture_sample at the reference's texture coordinates; Runner.evaluate / evaluate_sharded writing the per-sample files and
mesh_render.txt without changing any other output."""
import os

import numpy as np
import pytest
import torch

import mesh_raster_ref as ref
import texture_ref
from test_gpu_mesh_attributes import _opt, _sphere_level

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NEAR = 0.05
SIZES = ((16, 16), (20, 33), (33, 20))              # (H, W)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _px(points):
    """Screen points (x, y, z) in pixels and camera depth -> world points for identity pose and ref.pixel_intr(): (x z, y z, z)."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    return np.stack([p[:, 0] * p[:, 2], p[:, 1] * p[:, 2], p[:, 2]], axis=1).astype(np.float32)


def _hand_built():
    """{name: (verts [V,3] world fp32, faces [F,3] int32)} in the pixel units of _px, laid out for a 16 x 16 image (the larger sizes
    see the same meshes in their upper-left part)."""
    nan = np.nan
    fan_rim = [(13.5, 8.5), (12.0, 12.0), (8.5, 13.5), (5.0, 12.0), (3.5, 8.5), (5.0, 5.0), (8.5, 3.5), (12.0, 5.0)]
    tri = [(2.5, 2.5, 1), (12.5, 3.5, 1), (4.5, 12.5, 1)]
    m = {
        # the diagonal (2.5, 2.5) -> (10.5, 10.5) and the axis-parallel sides run through pixel centres
        "shared_edge": (_px([(2.5, 2.5, 1), (10.5, 2.5, 1), (10.5, 10.5, 2), (2.5, 10.5, 1)]), [[0, 1, 2], [0, 2, 3]]),
        "fan8": (_px([(8.5, 8.5, 1)] + [(x, y, 1 + 0.25 * (k % 3)) for k, (x, y) in enumerate(fan_rim)]),
                 [[0, 1 + k, 1 + (k + 1) % 8] if k % 2 else [1 + (k + 1) % 8, 0, 1 + k] for k in range(8)]),
        "sliver": (_px([(0.7, 1.2, 1), (15.2, 8.3, 1), (15.2, 8.9, 2)]), [[0, 1, 2]]),
        "zero_area": (_px([(1.5, 1.5, 1), (5.5, 5.5, 1), (9.5, 9.5, 1), (9.5, 1.5, 1)]), [[0, 1, 2], [0, 3, 2], [1, 1, 3]]),
        "off_sides": (_px([(-4, 3, 1), (3, 5, 1), (-2, 9, 1), (5, -6, 1), (9, 3, 1), (3, 2, 1), (40, 6, 1), (11, 4, 1), (12, 9, 1),
                           (6, 50, 1), (4, 11, 1), (9, 12, 1)]), [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11]]),
        "off_screen": (_px([(-10, -10, 1), (-5, -10, 1), (-10, -5, 1), (1e9, 3, 1), (1e9, 9, 1), (2e9, 5, 1)]), [[0, 1, 2], [3, 4, 5]]),
        "behind_near": (_px(tri + [(6.5, 6.5, 0.01), (7.5, 9.5, -1.0)]), [[0, 1, 2], [0, 1, 3], [4, 1, 2]]),
        "nan_vertex": (np.concatenate([_px(tri), np.array([[nan, 1, 1], [1, 1, np.inf]], np.float32)]), [[0, 1, 2], [0, 3, 2], [4, 1, 2], [3, 4, 0]]),
        "coincident": (_px(tri + tri), [[3, 4, 5], [0, 1, 2], [3, 4, 5]]),
        "stacked": (_px([(2.5, 2.5, 2), (12.5, 3.5, 2), (4.5, 12.5, 2), (5.5, 1.5, 1), (13.5, 8.5, 3), (1.5, 9.5, 1.5)]), [[0, 1, 2], [3, 4, 5]]),
        "front_back": (_px([(1.5, 1.5, 1), (7.5, 1.5, 1), (1.5, 7.5, 1), (8.5, 8.5, 1), (14.5, 8.5, 1), (8.5, 14.5, 1)]), [[0, 1, 2], [3, 5, 4]]),
    }
    out = {k: (np.asarray(v, np.float32), np.asarray(f, np.int32)) for k, (v, f) in m.items()}
    out["all"] = _concat(list(out.values()))
    return out


def _concat(meshes):
    verts, faces, base = [], [], 0
    for v, f in meshes:
        verts.append(v); faces.append(f + base); base += len(v)
    return np.concatenate(verts), np.concatenate(faces).astype(np.int32)


def _pack(meshes):
    """Per-image (verts, faces) -> the packed arguments of ops.mesh_raster: (verts, faces on the device, v_start, f_start, f_count)."""
    vc, fc = [len(v) for v, _ in meshes], [len(f) for _, f in meshes]
    v_start, f_start = [0] + np.cumsum(vc).tolist()[:-1], [0] + np.cumsum(fc).tolist()[:-1]
    verts = np.concatenate([np.asarray(v, np.float32).reshape(-1, 3) for v, _ in meshes])
    faces = np.concatenate([np.asarray(f, np.int32).reshape(-1, 3) for _, f in meshes])
    return _dev(verts), _dev(faces), v_start, f_start, fc


def _compare(meshes, pose, intr, H, W, out, near=NEAR):
    """Every (image, view) of `out` against the numpy restatement, bit for bit."""
    got = [t.cpu().numpy() for t in out]
    for b, (v, f) in enumerate(meshes):
        for k in range(pose.shape[1]):
            face, depth, bary, stats = ref.raster(v, f, pose[b, k], intr[b], H, W, near)
            assert np.array_equal(got[3][b, k], stats), (b, k, got[3][b, k], stats)
            assert np.array_equal(got[0][b, k], face), (b, k)
            assert np.array_equal(_bits(got[1][b, k]), _bits(depth)), (b, k)
            assert np.array_equal(_bits(got[2][b, k]), _bits(bary)), (b, k)


def _hand_cameras(B):
    """Two views per image: the identity (the meshes are in pixels) and a rolled, shifted camera (generic lattice points)."""
    pose = np.stack([ref.identity_pose(), ref.look_pose(0.0, 0.0, 0.1, 0.3) + np.array([[0, 0, 0, 0.3], [0, 0, 0, -0.2], [0, 0, 0, 0]], np.float32)])
    return np.broadcast_to(pose, (B, 2, 3, 4)).copy(), np.broadcast_to(ref.pixel_intr(), (B, 3, 3)).copy()


# ---- 1. bit for bit --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_hand_built_bit_for_bit(H, W):
    """Every rule of the header on a mesh of its own, and all of them in one image: shared edges and fan spokes through pixel centres,
    a sliver, zero area, faces hanging off each side, off-screen and out-of-range faces, a vertex behind `near`, NaN and Inf, coincident
    faces, faces at different depths, both windings."""
    from shapeclipper_amd import ops
    meshes = list(_hand_built().values())
    pose, intr = _hand_cameras(len(meshes))
    out = ops.mesh_raster(*_pack(meshes), _dev(pose), _dev(intr), H, W, NEAR)
    assert out.face.shape == (len(meshes), 2, H, W) and out.bary.shape == (len(meshes), 2, H, W, 3) and out.stats.shape == (len(meshes), 2, 4)
    _compare(meshes, pose, intr, H, W, out)
    named = dict(zip(_hand_built(), range(len(meshes))))
    face, stats = out.face.cpu().numpy(), out.stats.cpu().numpy()
    assert stats[named["zero_area"], 0].tolist() == [1, 0, 0, 2] and stats[named["behind_near"], 0].tolist() == [1, 2, 0, 0]
    assert stats[named["nan_vertex"], 0].tolist() == [1, 0, 3, 0] and stats[named["off_screen"], 0].tolist() == [1, 0, 1, 0]
    assert (face[named["off_screen"]] == -1).all()
    co = face[named["coincident"], 0]
    assert (co >= 0).sum() > 20 and (co[co >= 0] == 0).all()                     # the lower index wins the exact tie
    assert set(np.unique(face[named["front_back"], 0])) == {-1, 0, 1}             # both windings are drawn
    assert set(np.unique(face[named["stacked"], 0])) == {-1, 0, 1}
    assert len(np.unique(face[named["fan8"], 0])) == 9 and face[named["fan8"], 0][8, 8] >= 0


def test_real_meshes_bit_for_bit():
    """The marching-cubes meshes of the texture tests' batches ("a": sphere r = 0.3, "b": sphere r = 0.41, "e": empty, "2": two
    spheres at S = 32) at the positions the grid was sampled at, 3 perspective views of 32 x 32."""
    from shapeclipper_amd import ops
    H = W = 32
    for kinds, S in (("eab", 16), ("aeb", 16), ("2", 32)):
        grid = dict(a=lambda: texture_ref.sphere_level(S, 0.3), b=lambda: texture_ref.sphere_level(S, 0.41, (0.02, -0.03, 0.01)),
                    e=lambda: texture_ref.empty_level(S), **{"2": lambda: texture_ref.two_sphere_level(S)})
        verts, faces, vc, fc = ops.isosurface_mesh(_dev(np.stack([grid[k]() for k in kinds])))
        world = (np.float32(-0.5) + verts * np.float32(1.0 / (S - 1))).contiguous()
        v_end, f_end = np.cumsum(vc.numpy()).tolist(), np.cumsum(fc.numpy()).tolist()
        v_start, f_start = [0] + v_end[:-1], [0] + f_end[:-1]
        wn, fn = world.cpu().numpy(), faces.cpu().numpy()
        meshes = [(wn[v_start[b]:v_end[b]], fn[f_start[b]:f_end[b]]) for b in range(len(kinds))]
        B = len(kinds)
        pose = np.stack([np.stack([ref.look_pose(0.4 + b, 0.3 * k - 0.2, 2.2 + 0.4 * k, 0.5 * k) for k in range(3)]) for b in range(B)])
        intr = np.stack([ref.intrinsics(H, W, 1.5 + 0.25 * b) for b in range(B)])
        out = ops.mesh_raster(world, faces, v_start, f_start, fc.tolist(), _dev(pose), _dev(intr), H, W, NEAR)
        _compare(meshes, pose, intr, H, W, out)
        assert sum(fc.tolist()) > 500 and (out.face >= 0).sum().item() > 100 * (B - kinds.count("e"))
        assert (out.face[kinds.index("e")] == -1).all() if "e" in kinds else True


# ---- 2. memory, the two paths ----------------------------------------------------------------------------------------------------------
def test_nothing_is_written_outside_the_outputs():
    from shapeclipper_amd import _lib
    H, W = 20, 33
    meshes = [_hand_built()["all"], _hand_built()["fan8"]]
    pose, intr = _hand_cameras(2)
    verts, faces, v_start, f_start, fc = _pack(meshes)
    B, n_views, n, tail = 2, 2, 2 * 2 * H * W, 96
    face = torch.full((n + tail,), -7, dtype=torch.int32, device=DEV)
    depth, bary = torch.full((n + tail,), -7.0, device=DEV), torch.full((3 * n + tail,), -7.0, device=DEV)
    stats = torch.full((4 * B * n_views + tail,), -7, dtype=torch.int32, device=DEV)
    lib = _lib.load()
    n_bytes = lib.sc_mesh_raster_scratch_bytes(B, n_views, verts.shape[0], faces.shape[0], H, W)
    ws = torch.full((n_bytes + 256,), 0x5A, dtype=torch.uint8, device=DEV)
    starts = torch.tensor([v_start, f_start, fc], dtype=torch.int64, device=DEV)
    pose_d, intr_d = _dev(pose), _dev(intr)
    for large in (0, 64, 1 << 40):
        code = lib.sc_mesh_raster(_lib.ptr(verts), _lib.ptr(faces), _lib.ptr(starts[0]), _lib.ptr(starts[1]), _lib.ptr(starts[2]),
                                  _lib.ptr(pose_d), _lib.ptr(intr_d), B, verts.shape[0], faces.shape[0], n_views, H, W, NEAR,
                                  large, _lib.ptr(face), _lib.ptr(depth), _lib.ptr(bary), _lib.ptr(stats), _lib.ptr(ws), _lib.stream())
        assert code == 0
        assert (face[n:] == -7).all() and (depth[n:] == -7).all() and (bary[3 * n:] == -7).all() and (stats[4 * B * n_views:] == -7).all()
        assert (ws[n_bytes:] == 0x5A).all()
        out = (face[:n].view(B, n_views, H, W), depth[:n].view(B, n_views, H, W), bary[:3 * n].view(B, n_views, H, W, 3),
               stats[:4 * B * n_views].view(B, n_views, 4))
        _compare(meshes, pose, intr, H, W, out)


def test_both_paths_agree():
    """large_pixels = 0 (every face by a wave), 64 and 2^40 (every face by its own thread): identical bytes, on the hand-built meshes
    (boxes of up to the whole image) and on a marching-cubes sphere."""
    from shapeclipper_amd import ops
    meshes = list(_hand_built().values())
    pose, intr = _hand_cameras(len(meshes))
    packed = _pack(meshes)
    for H, W in ((33, 20), (64, 48)):
        outs = [ops.mesh_raster(*packed, _dev(pose), _dev(intr), H, W, NEAR, large_pixels=lp) for lp in (0, 64, 1 << 40)]
        for o in outs[1:]:
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs[0], o))
        assert (outs[0].face >= 0).sum().item() > 300
    world, faces, args, pose, intr = _device_sphere(2)
    outs = [ops.mesh_raster(world, faces, *args, pose, intr, 48, 40, NEAR, large_pixels=lp) for lp in (0, 3, 64, 1 << 40)]
    for o in outs[1:]:
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs[0], o))


def _device_sphere(n_views, H=48, W=40):
    """The device mesh (ops.isosurface_mesh) of the shell tests' sphere at its sampled positions, with n_views cameras."""
    from shapeclipper_amd import ops
    s = ref.SHELL_SPHERE
    verts, faces, vc, fc = ops.isosurface_mesh(_dev(texture_ref.sphere_level(s["S"], s["radius"], s["centre"])[None]))
    world = (np.float32(-0.5) + verts * np.float32(1.0 / (s["S"] - 1))).contiguous()
    pose = np.stack([ref.look_pose(0.9 * k + 0.2, 0.4 - 0.3 * k, 3.0 + k, 0.7 * k) for k in range(n_views)])[None]
    intr = ref.intrinsics(H, W, 3.0)[None]
    return world, faces, ([0], [0], fc.tolist()), _dev(pose), _dev(intr)


# ---- 3. partition -----------------------------------------------------------------------------------------------------------------------
def test_one_face_per_image_partitions_the_mask():
    """Meshes that do not overlap themselves on the screen (the fan, the quad, a jittered height field seen in perspective), rendered
    once whole and once as F images of one face each: the F masks are pairwise disjoint and their union is the whole mesh's mask;
    every one-face image names face 0 where the whole mesh names that face."""
    from shapeclipper_amd import ops
    rng = np.random.RandomState(5)
    n = 7
    gx, gy = np.meshgrid(np.arange(n), np.arange(n), indexing="xy")
    sx = 2.5 + 4.0 * gx + np.rint(rng.uniform(-1, 1, gx.shape) * 2) / 2           # half-pixel lattice: edges through centres
    sy = 1.5 + 4.0 * gy + np.rint(rng.uniform(-1, 1, gy.shape) * 2) / 2
    field = _px(np.stack([sx, sy, rng.choice([1.0, 2.0, 4.0], gx.shape)], axis=-1))
    quad = lambda a: [[a, a + 1, a + n + 1], [a, a + n + 1, a + n]] if (a // n + a) % 2 else [[a, a + 1, a + n], [a + 1, a + n + 1, a + n]]
    field_faces = np.array([t for r in range(n - 1) for c in range(n - 1) for t in quad(r * n + c)], np.int32)
    hb = _hand_built()
    H, W = 30, 31
    for verts, faces in (hb["fan8"], hb["shared_edge"], (field, field_faces)):
        F = len(faces)
        pose, intr = _hand_cameras(F)
        whole = ops.mesh_raster(*_pack([(verts, faces)]), _dev(pose[:1]), _dev(intr[:1]), H, W, NEAR)
        single = ops.mesh_raster(*_pack([(verts[f], np.array([[0, 1, 2]], np.int32)) for f in faces]), _dev(pose), _dev(intr), H, W, NEAR)
        masks = single.face >= 0                                                   # [F, 2, H, W]
        assert masks.sum(dim=0).max().item() == 1
        assert torch.equal(masks.any(dim=0), whole.face[0] >= 0)
        assert torch.equal(masks.long().argmax(dim=0)[masks.any(dim=0)], whole.face[0].long()[whole.face[0] >= 0])
        assert masks.any(dim=0).sum().item() > (40 if F < 10 else 400)


# ---- 4. the derived shells on the device mesh -------------------------------------------------------------------------------------------
def test_device_sphere_between_shells():
    """tests/test_mesh_raster_host.py's shell test on ops.isosurface_mesh's mesh and the kernel's output: the same views, bounds and cap."""
    from shapeclipper_amd import ops
    s = ref.SHELL_SPHERE
    verts, faces, vc, fc = ops.isosurface_mesh(_dev(texture_ref.sphere_level(s["S"], s["radius"], s["centre"])[None]))
    pitch = 1.0 / (s["S"] - 1)
    world = (np.float32(-0.5) + verts * np.float32(pitch)).contiguous()
    for H, W, dist, pose in ref.SHELL_VIEWS:
        intr = ref.intrinsics(H, W, 4.0)
        out = ops.mesh_raster(world, faces, [0], [0], fc.tolist(), _dev(pose[None, None]), _dev(intr[None]), H, W, NEAR)
        assert out.stats[0, 0, 1:3].tolist() == [0, 0]
        hit, miss, undecided, bad = ref.shell_check(out.face[0, 0].cpu().numpy(), out.depth[0, 0].cpu().numpy(), pose, intr, s["centre"],
                                                    s["radius"], pitch, "device")
        assert bad == 0
        assert hit > 50 and miss > 50 and undecided <= 0.05 * H * W


# ---- 5. determinism and invariance -------------------------------------------------------------------------------------------------------
def test_determinism_batch_and_view_invariance():
    from shapeclipper_amd import ops
    hb = _hand_built()
    meshes = [hb["all"], hb["fan8"], (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)), hb["stacked"]]
    H, W = 33, 20
    rng = np.random.RandomState(2)
    pose = np.stack([np.stack([ref.look_pose(0.0, 0.0, 0.05 * k, 0.4 * k + b) + np.array([[0, 0, 0, 0.5 * k], [0, 0, 0, 0.25 * b], [0, 0, 0, 0]],
                                                                                              np.float32) for k in range(4)]) for b in range(4)])
    intr = np.broadcast_to(ref.pixel_intr(), (4, 3, 3)).copy()
    same = lambda a, b: all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    first = ops.mesh_raster(*_pack(meshes), _dev(pose), _dev(intr), H, W, NEAR)
    keep = [t.clone() for t in first]
    for lp in (64, 0):                                                  # (the second run reuses the first one's scratch)
        assert same(keep, ops.mesh_raster(*_pack(meshes), _dev(pose), _dev(intr), H, W, NEAR, large_pixels=lp))
    assert (keep[0][2] == -1).all() and (keep[3][2] == 0).all()         # the image without faces
    for b in range(4):                                                  # alone
        alone = ops.mesh_raster(*_pack(meshes[b:b + 1]), _dev(pose[b:b + 1]), _dev(intr[b:b + 1]), H, W, NEAR)
        assert same([t[b:b + 1] for t in keep], alone), b
    perm = rng.permutation(4)
    permuted = ops.mesh_raster(*_pack(meshes), _dev(pose[:, perm]), _dev(intr), H, W, NEAR)
    assert same([t[:, list(perm)] for t in keep], permuted)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from shapeclipper_amd import ops
    hb = _hand_built()
    verts, faces, v_start, f_start, fc = _pack([hb["fan8"], hb["stacked"]])
    pose, intr = (_dev(a) for a in _hand_cameras(2))
    ok = lambda **kw: ops.mesh_raster(kw.get("verts", verts), kw.get("faces", faces), kw.get("v", v_start), kw.get("f", f_start),
                                      kw.get("c", fc), kw.get("pose", pose), kw.get("intr", intr), kw.get("H", 16), kw.get("W", 16),
                                      kw.get("near", NEAR), **({"large_pixels": kw["lp"]} if "lp" in kw else {}))
    ok()
    for bad in (dict(H=0), dict(W=4097), dict(H=16.0), dict(near=0.0), dict(near=-1.0), dict(near=float("nan")), dict(near=None), dict(lp=-1),
                dict(lp=2.5), dict(pose=pose[:1]), dict(pose=pose[:, :0]), dict(pose=pose[..., :3]), dict(intr=intr[:1]), dict(intr=intr[:, :2]),
                dict(pose=pose.double()), dict(pose=pose.cpu()), dict(verts=verts.cpu()), dict(faces=faces.long()), dict(verts=verts[:, :2]),
                dict(v=[0, verts.shape[0] + 1]), dict(v=[5, 0]), dict(v=[0]), dict(f=[0, faces.shape[0]]), dict(f=[0, fc[0] - 1]),
                dict(c=[fc[0], fc[1] + 1]), dict(c=[fc[0], -1]), dict(v=[0, 0])):
        with pytest.raises(ValueError):
            ok(**bad)
    with pytest.raises(ValueError):                                     # more than 65535 images
        n = 65536
        ops.mesh_raster(verts, faces, [0] * n, [0] * n, [0] * n, pose[:1].expand(n, -1, -1, -1), intr[:1].expand(n, -1, -1), 1, 1, NEAR)


# ---- 7. eval_3D.mesh_render -------------------------------------------------------------------------------------------------------------
def _networks(extra=(), seed=1):
    from shapeclipper_amd.model.implicit import RGBNetwork, SDFNetwork
    opt = _opt(["--eval.vox_res=16", *extra])
    torch.manual_seed(seed)
    sdf_net, rgb_net = SDFNetwork(opt), RGBNetwork(opt)
    with torch.no_grad():                                                       # (the SDF keeps its geometric init: a sphere)
        for p in rgb_net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return opt, sdf_net.to(DEV), rgb_net.to(DEV)


def test_mesh_render_colours_are_the_viewers_lookup():
    """Random networks, three images (the middle one empty), two views, 40 x 36 pixels from intrinsics given for opt.H x opt.W: face,
    depth and barycentrics are the numpy restatement's for the mesh at its sampled positions and the rescaled intrinsics; at covered
    pixels colour and normal equal ops.texture_sample of the atlases at the reference's uv = (b0 vt0 + b1 vt1) + b2 vt2, / 255, bit for
    bit; misses are data.bgcolor and mid-grey; the orthographic camera is refused by name."""
    from shapeclipper_amd import ops
    from shapeclipper_amd.utils import camera, eval_3D
    opt, sdf_net, rgb_net = _networks(["--eval.texture_texels=5"])
    g = torch.Generator().manual_seed(7)
    B, V, H, W = 3, 2, 40, 36
    zs, zr = (0.15 * torch.randn(B, 64, generator=g)).to(DEV), torch.randn(B, 64, generator=g).to(DEV)
    level = _sphere_level(opt, sdf_net, zs)
    level[1] = 1.0
    level[2] += 0.12
    textured = eval_3D.mesh_texture(opt, sdf_net, rgb_net, zs, zr, level)
    opt.H, opt.W = 64, 64
    intr = camera.get_intr(opt, torch.tensor([1.0, 1.1, 0.9])).to(DEV)
    pose = np.stack([np.stack([ref.look_pose(0.5 + b, 0.3 - 0.5 * k, 4.6 + 0.3 * b, 0.2 * k) for k in range(V)]) for b in range(B)])
    out = eval_3D.mesh_render(opt, level, textured, _dev(pose), intr, H, W)
    assert out.rgb.shape == out.normal.shape == (B, V, H, W, 3) and out.mask.shape == out.depth.shape == out.face.shape == (B, V, H, W)
    # the raster: the sampled positions, diag(W / opt.W, H / opt.H, 1) @ intr
    lo, hi = opt.eval.range
    S = level.shape[1]
    verts, faces, vc, fc = ops.isosurface_mesh(level)
    world = (lo + verts * ((hi - lo) / (S - 1))).cpu().numpy()
    v_end, f_end = np.cumsum(vc.numpy()).tolist(), np.cumsum(fc.numpy()).tolist()
    meshes = [(world[v_end[b] - int(vc[b]):v_end[b]], faces[f_end[b] - int(fc[b]):f_end[b]].cpu().numpy()) for b in range(B)]
    k = (intr * torch.tensor([W / 64, H / 64, 1.0], device=DEV).view(1, 3, 1)).cpu().numpy()
    _compare(meshes, pose, k, H, W, (out.face, out.depth, out.bary, out.stats), near=eval_3D.MESH_RENDER_NEAR)
    assert int(fc[0]) > 100 and int(fc[1]) == 0 and (out.face[1] == -1).all() and (out.mask == (out.face >= 0).float()).all()
    A = textured[0].atlas.shape[0]
    for b in (0, 2):
        face, bary = out.face[b].cpu().numpy(), out.bary[b].cpu().numpy()
        ok = face >= 0
        assert ok.sum() > 150
        vt = texture_ref.face_uv(int(fc[b]), A, 5).astype(np.float32)[face[ok]]                 # [n,3,2]
        t = bary[ok][:, :, None] * vt
        uv = (t[:, 0] + t[:, 1]) + t[:, 2]
        image = torch.zeros(len(uv), dtype=torch.int32, device=DEV)
        for got, atlas in ((out.rgb, textured[b].atlas), (out.normal, textured[b].normal_atlas)):
            looked = ops.texture_sample(atlas[None].contiguous(), _dev(uv), image)
            assert torch.equal(got[b][_dev(ok)].view(torch.int32), (looked / 255).view(torch.int32)), b
            assert np.array_equal(_bits(looked.cpu().numpy()), _bits(texture_ref.sample(atlas.cpu().numpy(), uv)))
        assert (out.rgb[b][_dev(~ok)] == float(opt.data.bgcolor)).all() and (out.normal[b][_dev(~ok)] == 0.5).all()
        assert (out.depth[b][_dev(~ok)] == 0).all() and (out.depth[b][_dev(ok)] > 3).all()
    assert (out.rgb[1] == float(opt.data.bgcolor)).all() and (out.normal[1] == 0.5).all()
    # [B,3,4] poses are one view; the thread and the wave path draw the same picture
    one = eval_3D.mesh_render(opt, level, textured, _dev(pose[:, 1]), intr, H, W, large_pixels=0)
    assert all(torch.equal(a[:, 1:].view(torch.int32), b.view(torch.int32)) for a, b in zip(out, one))
    opt.camera.model = "orthographic"
    with pytest.raises(NotImplementedError, match="camera.model"):
        eval_3D.mesh_render(opt, level, textured, _dev(pose), intr, H, W)


def test_mask_iou_is_exact():
    from shapeclipper_amd.utils import eval_3D
    a = torch.zeros(3, 5, 7, dtype=torch.bool, device=DEV)
    b = torch.zeros(3, 5, 7, dtype=torch.bool, device=DEV)
    a[0, :2] = True; b[0, 1:4] = True           # 14 and 21 pixels, 7 shared: 7 / 28
    a[1, 0, 0] = True                           # disjoint from an empty mask: 0
    got = eval_3D.mask_iou(a, b)
    assert got.dtype == torch.float64 and got.tolist() == [0.25, 0.0, 1.0]      # an empty union gives 1


# ---- 8. the evaluation's dumps ---------------------------------------------------------------------------------------------------------
MESH_SUFFIXES = ("_image_mesh.png", "_mask_mesh.png", "_normal_mesh.png", "_depth_mesh.png", "_depth_mesh.npy")


def test_evaluate_writes_mesh_renders(tmp_path):
    """Runner.evaluate (plain) and evaluate_sharded (combined with --hip.largest_component): with --eval.mesh_render the five files per
    sample and mesh_render.txt appear -- IoUs in [0, 1] or nan, `pixels` the mask PNG's count, the depth file the mask's support --;
    without --eval.texture no OBJ and no texture.txt is written; with the switch off none of the new files appear and every other file
    has the same bytes.  The vis_{ep}/ dump of the training-time visualisation gets the pictures and the two turn-table GIFs."""
    PIL = pytest.importorskip("PIL.Image")
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    from copy import deepcopy
    from shapeclipper_amd.model.runner import Runner
    from shapeclipper_amd.utils import eval_3D
    from shapeclipper_amd.utils.util import EasyDict as edict
    o = _opt(["--arch.enc_pretrained!", "--data.dataset=synthetic", "--eval.vox_res=16", "--eval.num_points=1000", "--tb!", "--eval.mesh_render"],
             output_root=str(tmp_path))
    o.device, o.world_size, o.port = 0, 1, 0
    torch.manual_seed(0)
    r = Runner(o)
    r.load_dataset(o, eval_split="test")
    r.build_networks(o)
    out = os.path.join(o.output_path, "dump")

    def snapshot():
        files = {os.path.join("dump", f): open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}
        files.update({f: open(os.path.join(o.output_path, f), "rb").read() for f in sorted(os.listdir(o.output_path)) if f.endswith(".txt")})
        return files

    def clear():
        for f in os.listdir(out) if os.path.isdir(out) else []:
            os.remove(os.path.join(out, f))
        for f in os.listdir(o.output_path):
            if f.endswith(".txt"):
                os.remove(os.path.join(o.output_path, f))

    is_new = lambda name: name == "mesh_render.txt" or name.endswith(MESH_SUFFIXES)
    n_samples = len(r.test_data)
    Hm, Wm = o.image_size                               # the size of var.mask_input_map: the input picture's, not the evaluation render's
    assert tuple(o.image_size) != tuple(o.eval.image_size)
    for mode, largest in (("evaluate", False), ("evaluate_sharded", True)):
        o.hip.largest_component = largest
        clear()
        o.eval.mesh_render = True
        getattr(r, mode)(o, ep=0)
        on = snapshot()
        rows = [l.split() for l in on["mesh_render.txt"].decode().splitlines()]
        assert [int(x[0]) for x in rows] == list(range(n_samples)) and all(len(x) == 5 for x in rows)
        assert not any(k.endswith((".obj", ".mtl")) or "_mesh_tex" in k or k == "texture.txt" for k in on)       # --eval.texture is off
        drawn = 0
        for x in rows:
            i, faces, pixels = (int(v) for v in x[:3])
            for iou in (float(x[3]), float(x[4])):
                assert np.isnan(iou) or 0.0 <= iou <= 1.0
            for suffix in MESH_SUFFIXES:
                assert os.path.join("dump", "%d%s" % (i, suffix)) in on
            mask = np.asarray(PIL.open(os.path.join(out, "%d_mask_mesh.png" % i)))
            image = np.asarray(PIL.open(os.path.join(out, "%d_image_mesh.png" % i)))
            depth = np.load(os.path.join(out, "%d_depth_mesh.npy" % i))
            assert mask.shape == depth.shape == (Hm, Wm) and image.shape == (Hm, Wm, 3) and set(np.unique(mask)) <= {0, 255}
            assert (mask == 255).sum() == pixels and np.array_equal(depth > 0, mask == 255) and depth.dtype == np.float32
            assert (image[mask == 0] == int(255 * float(o.data.bgcolor))).all()
            if faces == 0:
                assert pixels == 0
            drawn += pixels
        assert drawn > 0, mode
        # the switch off: none of the new files, every other file byte-identical
        clear()
        o.eval.mesh_render = False
        getattr(r, mode)(o, ep=0)
        off = snapshot()
        assert not any(is_new(os.path.basename(k)) for k in off)
        assert off == {k: v for k, v in on.items() if not is_new(os.path.basename(k))}
        assert ("components.txt" in off) == largest
    # with --eval.texture as well the OBJ files and texture.txt come back, and mesh_render.txt keeps its bytes (var.texture is shared)
    o.hip.largest_component = False
    clear()
    o.eval.mesh_render, o.eval.texture = True, True
    r.evaluate(o, ep=0)
    both = snapshot()
    assert "texture.txt" in both and os.path.join("dump", "0_mesh_tex.obj") in both
    clear()
    o.eval.texture = False
    r.evaluate(o, ep=0)
    assert snapshot()["mesh_render.txt"] == both["mesh_render.txt"]
    # vis_{ep}/ of --hip.train_vis: the per-sample pictures through dump_geometry, the GIFs from one raster call over var.vis_pose
    r.graph.eval()
    o.H, o.W = o.eval.image_size
    os.makedirs(os.path.join(o.output_path, "vis_3"), exist_ok=True)
    sample = r.test_data[0]
    batch = {k: ({kk: vv[None] for kk, vv in v.items()} if isinstance(v, dict) else torch.as_tensor(v)[None]) for k, v in sample.items()}
    from shapeclipper_amd import ops
    calls, raster = [], ops.mesh_raster
    with torch.no_grad():
        var = r.evaluate_batch(o, edict(batch), 0, 0, single_gpu=True)
        var = r.graph.module.get_rotate_pose(o, var, n_views=5)
        eval_3D.eval_metrics(o, var, r.graph.module.sdf_network, vis_only=True)
        r.dump_geometry(o, var, "vis_3")
        ops.mesh_raster = lambda *a, **k: calls.append(a[5].shape) or raster(*a, **k)
        try:
            r.dump_mesh_turntable(o, var, "vis_3")
        finally:
            ops.mesh_raster = raster
    assert calls == [(1, 5, 3, 4)]                                      # all of var.vis_pose in one call
    names = os.listdir(os.path.join(o.output_path, "vis_3"))
    i = int(var.idx[0])
    assert all("%d%s" % (i, s) in names for s in MESH_SUFFIXES + ("_image_mesh_rotate.gif", "_normal_mesh_rotate.gif"))
    gif = PIL.open(os.path.join(o.output_path, "vis_3", "%d_image_mesh_rotate.gif" % i))
    assert gif.n_frames == 5 and gif.size == (Wm, Hm)
