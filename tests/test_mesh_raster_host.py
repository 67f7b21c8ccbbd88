"""The rasteriser's rules on the host (tests/mesh_raster_ref.py, the numpy restatement of include/shapeclipper_hip.h): the top-left
rule partitions the pixel centres of a fan, and a marching-cubes sphere rendered through a perspective camera lies between two
derived shells.  No GPU."""
import numpy as np

import mesh_raster_ref as ref
import texture_ref


def test_fans_are_partitioned():
    """116 seeded fans of 3..8 triangles, the hub on a pixel centre, the rim on the half-pixel lattice, windings flipped at random: no
    pixel centre is covered twice, the hub's pixel exactly once, and every centre strictly inside the fan's outline at least once."""
    rng = np.random.RandomState(11)
    on_edge = 0
    for k in range(116):
        n_tri = 3 + k % 6
        H, W = (24, 31) if k % 2 else (32, 32)
        X, Y, faces, (ci, cj) = ref.fan(rng, n_tri, H, W)
        z = np.ones(len(X), np.float32)
        face, depth, bary, stats, covers = ref.raster_lattice(X, Y, z, np.zeros(len(X), np.int64), faces, H, W, count=True)
        assert stats.tolist() == [n_tri, 0, 0, 0]
        assert covers.max() == 1, (k, "a pixel centre is covered twice")
        assert covers[cj, ci] == 1 and face[cj, ci] >= 0, (k, "the hub")
        assert np.array_equal(covers == 1, face >= 0)
        # the union: a centre strictly inside a wedge (all three edge functions of the hub -> rim k -> rim k+1 triangle positive) is covered
        rx, ry = X[1:], Y[1:]
        nx, ny = np.roll(rx, -1), np.roll(ry, -1)
        j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        Px, Py = 256 * i + 128, 256 * j + 128
        inside = np.zeros((H, W), bool)
        for t in range(n_tri):
            e0 = (rx[t] - X[0]) * (Py - Y[0]) - (ry[t] - Y[0]) * (Px - X[0])
            e1 = (nx[t] - rx[t]) * (Py - ry[t]) - (ny[t] - ry[t]) * (Px - rx[t])
            e2 = (X[0] - nx[t]) * (Py - ny[t]) - (Y[0] - ny[t]) * (Px - nx[t])
            inside |= (e0 > 0) & (e1 > 0) & (e2 > 0)
            on_edge += int(((e0 == 0) & (e1 > 0) & (e2 >= 0)).sum())
        assert (covers[inside] == 1).all()
        ok = face >= 0
        # every z is 1: b_k rounds three times (two conversions, a quotient; the b_k sum to 1), the sum twice, the reciprocal once
        assert (np.abs(depth[ok] - 1) <= 6 * 2.0 ** -24).all() and (np.abs(bary[ok].sum(axis=1) - 1) <= 8 * 2.0 ** -24).all()
        assert (bary[~ok] == 0).all() and (depth[~ok] == 0).all() and (bary[ok] >= 0).all()
    assert on_edge > 200                                # the fans do run their spokes through pixel centres


def test_coincident_and_stacked_faces():
    """Two coincident faces: the lower index wins.  A nearer face over a farther one wins whatever its index."""
    X, Y = np.array([256, 2816, 256], np.int64), np.array([256, 256, 2816], np.int64)
    tri = np.array([[0, 1, 2]])
    both = np.concatenate([tri, tri[:, [0, 2, 1]]])
    face, *_ = ref.raster_lattice(X, Y, np.ones(3, np.float32), np.zeros(3, np.int64), both, 12, 12)
    assert (face >= 0).sum() > 20 and (face[face >= 0] == 0).all()
    X2, Y2 = np.concatenate([X, X]), np.concatenate([Y, Y])
    z2 = np.array([2, 2, 2, 1, 1, 1], np.float32)
    face, depth, *_ = ref.raster_lattice(X2, Y2, z2, np.zeros(6, np.int64), np.array([[0, 1, 2], [3, 4, 5]]), 12, 12)
    assert (face[face >= 0] == 1).all() and (depth[face >= 0] == 1).all()


def test_sphere_between_shells():
    """The oracle's marching-cubes mesh of a sphere, two views: every ray that hits the inner shell is covered at a depth between the
    two shells' entry depths, every ray that misses the outer shell is a miss, and at most 5 % of the pixels are undecided
    (ref.shell_check derives the shells)."""
    from oracle import isosurface_ref
    s = ref.SHELL_SPHERE
    level = texture_ref.sphere_level(s["S"], s["radius"], s["centre"])
    verts, faces = ref.index_triangles(isosurface_ref.marching_cubes(level))
    pitch = 1.0 / (s["S"] - 1)
    world = (np.float32(-0.5) + verts * np.float32(pitch)).astype(np.float32)
    assert len(faces) > 300
    for H, W, dist, pose in ref.SHELL_VIEWS:
        intr = ref.intrinsics(H, W, 4.0)
        face, depth, bary, stats = ref.raster(world, faces, pose, intr, H, W, 0.05)
        assert stats.tolist()[1:3] == [0, 0] and stats[0] + stats[3] == len(faces)
        hit, miss, undecided, bad = ref.shell_check(face, depth, pose, intr, s["centre"], s["radius"], pitch, "host")
        assert bad == 0
        assert hit > 50 and miss > 50 and undecided <= 0.05 * H * W


def test_mesh_render_switch_is_validated():
    """eval.mesh_render: absent means off; anything but a bool is a ValueError, whether the switch would be on or not."""
    import pytest
    from shapeclipper_amd.utils import options
    from shapeclipper_amd.utils.util import EasyDict as edict
    assert options.mesh_render(edict(eval=edict(vox_res=64))) is False and options.mesh_render(edict()) is False
    assert options.mesh_render(edict(eval=edict(mesh_render=True))) is True and options.mesh_render(edict(eval=edict(mesh_render=False))) is False
    for bad in (1, 0, "true", None, 0.5):
        with pytest.raises(ValueError, match="eval.mesh_render"):
            options.mesh_render(edict(eval=edict(mesh_render=bad)))
    opt = options.parse_arguments(["--yaml=options/pix3d/config.yaml", "--name=pytest_mesh_render", "--output_root=/tmp/sc_pytest", "--eval.mesh_render"])
    assert options.set(opt, verbose=False).eval.mesh_render is True
    with pytest.raises(ValueError, match="eval.mesh_render"):
        options.set(options.parse_arguments(["--yaml=options/pix3d/config.yaml", "--name=pytest_mesh_render", "--output_root=/tmp/sc_pytest",
                                             "--eval.mesh_render=3"]), verbose=False)
