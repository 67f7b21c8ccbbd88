"""numpy restatement of the triangle rasteriser (include/shapeclipper_hip.h: sc_mesh_raster) and the meshes, cameras and derived
bounds its tests share.  Not a test module.

Coverage is int64 arithmetic; everything the kernels compute in fp32 is computed here in np.float32, one operation per line where the
order matters, so the GPU tests compare bit for bit.  One image and one view at a time; the callers loop."""
import numpy as np

F32 = np.float32
I64 = np.int64
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
SNAP_LIMIT = F32(2.0 ** 28)
F32_MAX = np.finfo(np.float32).max
DRAWN, CULL_NEAR, CULL_RANGE, ZERO_AREA = 0, 1, 2, 3


def project(verts, pose, intr, near):
    """verts [V,3], pose [3,4] world-to-camera, intr [3,3] -> (X, Y int64 [V] on the 1/256-pixel lattice, zc fp32 [V], flag [V]):
    the header's per-vertex block.  flag: 0, CULL_NEAR or CULL_RANGE; X = Y = 0 where the flag is set."""
    v, P, K = np.asarray(verts, F32).reshape(-1, 3), np.asarray(pose, F32), np.asarray(intr, F32)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        cam = []
        for r in range(3):
            t0 = P[r, 0] * x
            t1 = P[r, 1] * y
            t2 = P[r, 2] * z
            cam.append(((t0 + t1) + t2) + P[r, 3])
        xc, yc, zc = cam
        sx = (K[0, 0] * xc) / zc + K[0, 2]
        sy = (K[1, 1] * yc) / zc + K[1, 2]
        fx, fy = np.rint(sx * F32(256)), np.rint(sy * F32(256))
        is_near = zc < F32(near)
        bad = ~(np.abs(zc) <= F32_MAX) | ~(np.abs(fx) < SNAP_LIMIT) | ~(np.abs(fy) < SNAP_LIMIT)
    flag = np.where(is_near, CULL_NEAR, np.where(bad, CULL_RANGE, DRAWN))
    ok = flag == DRAWN
    X = np.where(ok, np.nan_to_num(fx, nan=0.0, posinf=0.0, neginf=0.0), 0).astype(I64)
    Y = np.where(ok, np.nan_to_num(fy, nan=0.0, posinf=0.0, neginf=0.0), 0).astype(I64)
    return X, Y, zc.astype(F32), flag


def _edge(px, py, qx, qy, Px, Py):
    dx, dy = qx - px, qy - py
    E = dx * (Py - py) - dy * (Px - px)
    return E, (E > 0) | ((E == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))


def _shade(ox, oy, oz, area, i, j):
    """Oriented triangles (ox, oy [n,3] int64, oz [n,3] fp32, area [n] > 0) at pixels (i, j) [n] -> (covered, depth, bary oriented)."""
    Px, Py = 256 * i.astype(I64) + 128, 256 * j.astype(I64) + 128
    E2, in2 = _edge(ox[:, 0], oy[:, 0], ox[:, 1], oy[:, 1], Px, Py)
    E0, in0 = _edge(ox[:, 1], oy[:, 1], ox[:, 2], oy[:, 2], Px, Py)
    E1, in1 = _edge(ox[:, 2], oy[:, 2], ox[:, 0], oy[:, 0], Px, Py)
    covered = in0 & in1 & in2
    fa = area.astype(F32)
    with np.errstate(all="ignore"):
        b = [E.astype(F32) / fa for E in (E0, E1, E2)]
        q = [b[k] / oz[:, k] for k in range(3)]
        s = (q[0] + q[1]) + q[2]
        depth = F32(1) / s
        bary = np.stack([q[k] / s for k in range(3)], axis=1)
    return covered, depth.astype(F32), bary.astype(F32)


def raster_lattice(X, Y, zc, flag, faces, H, W, count=False):
    """The per-face, visibility and resolve blocks on projected vertices -> (face [H,W] int32, depth [H,W] fp32, bary [H,W,3] fp32,
    stats [4] int32); count=True adds covers [H,W], the number of faces covering each pixel centre."""
    V = len(X)
    faces = np.asarray(faces, I64).reshape(-1, 3)
    face_out, depth_out = np.full((H, W), -1, np.int32), np.zeros((H, W), F32)
    bary_out, stats, covers = np.zeros((H, W, 3), F32), np.zeros(4, np.int32), np.zeros((H, W), np.int64)
    done = lambda: (face_out, depth_out, bary_out, stats) + ((covers,) if count else ())
    if len(faces) == 0:
        return done()
    assert V > 0, "an image with faces has vertices"
    fv = np.clip(faces, 0, V - 1)
    fl = flag[fv]
    cat = np.where((fl == CULL_NEAR).any(axis=1), CULL_NEAR, np.where((fl == CULL_RANGE).any(axis=1), CULL_RANGE, DRAWN))
    x, y, z = X[fv], Y[fv], zc[fv]
    area = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
    cat = np.where((cat == DRAWN) & (area == 0), ZERO_AREA, cat)
    stats[:] = [(cat == c).sum() for c in range(4)]
    swapped = area < 0
    order = np.where(swapped[:, None], np.array([0, 2, 1]), np.array([0, 1, 2]))         # oriented vertex k is the face's order[k]
    rows = np.arange(len(faces))[:, None]
    ox, oy, oz, area = x[rows, order], y[rows, order], z[rows, order], np.abs(area)
    i0 = np.maximum((ox.min(axis=1) + 127) >> 8, 0)
    i1 = np.minimum((ox.max(axis=1) - 128) >> 8, W - 1)
    j0 = np.maximum((oy.min(axis=1) + 127) >> 8, 0)
    j1 = np.minimum((oy.max(axis=1) - 128) >> 8, H - 1)
    bw, bh = np.where(cat == DRAWN, i1 - i0 + 1, 0), np.where(cat == DRAWN, j1 - j0 + 1, 0)
    live = (bw > 0) & (bh > 0)
    keys = np.full(H * W, EMPTY, np.uint64)
    for dj in range(int(bh[live].max()) if live.any() else 0):
        for di in range(int(bw[live].max())):
            f = np.nonzero(live & (di < bw) & (dj < bh))[0]
            if len(f) == 0:
                continue
            i, j = i0[f] + di, j0[f] + dj
            covered, depth, _ = _shade(ox[f], oy[f], oz[f], area[f], i, j)
            f, pix, depth = f[covered], (j * W + i)[covered], depth[covered]
            np.add.at(covers.reshape(-1), pix, 1)
            np.minimum.at(keys, pix, (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | f.astype(np.uint64))
    pix = np.nonzero(keys != EMPTY)[0]
    if len(pix):
        f = (keys[pix] & np.uint64(0xFFFFFFFF)).astype(I64)
        covered, depth, bary = _shade(ox[f], oy[f], oz[f], area[f], pix % W, pix // W)
        assert covered.all() and np.array_equal(depth.view(np.uint32).astype(np.uint64), keys[pix] >> np.uint64(32))
        own = np.empty_like(bary)
        own[np.arange(len(f))[:, None], order[f]] = bary                                    # back into the face's own slots
        face_out.reshape(-1)[pix], depth_out.reshape(-1)[pix], bary_out.reshape(-1, 3)[pix] = f, depth, own
    return done()


def raster(verts, faces, pose, intr, H, W, near):
    """One image from one view: the whole of sc_mesh_raster -> (face, depth, bary, stats)."""
    return raster_lattice(*project(verts, pose, intr, near), faces, H, W)


# ---- cameras ------------------------------------------------------------------------------------------------------------------------
def intrinsics(H, W, focal):
    """camera.get_intr's matrix: [[f W, 0, W / 2], [0, f H, H / 2], [0, 0, 1]], fp32."""
    return np.array([[focal * W, 0, W / 2], [0, focal * H, H / 2], [0, 0, 1]], F32)


def look_pose(azim, elev, dist, roll=0.0):
    """World-to-camera [3,4] fp32: rotations about y, x and z, then the object pushed `dist` down the camera's z axis."""
    ca, sa, ce, se, cr, sr = np.cos(azim), np.sin(azim), np.cos(elev), np.sin(elev), np.cos(roll), np.sin(roll)
    Ry = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]])
    Rx = np.array([[1, 0, 0], [0, ce, -se], [0, se, ce]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return np.concatenate([Rz @ Rx @ Ry, np.array([[0.0], [0.0], [dist]])], axis=1).astype(F32)


def identity_pose(dist=0.0):
    return np.concatenate([np.eye(3), np.array([[0.0], [0.0], [dist]])], axis=1).astype(F32)


def pixel_intr():
    """Screen coordinates = camera x / z and y / z: with vertices at z = 1 a mesh is given in pixels directly."""
    return np.eye(3, dtype=F32)


# ---- fans: the partition property of the top-left rule --------------------------------------------------------------------------------
def fan(rng, n_tri, H, W):
    """A closed fan of n_tri triangles around a hub that sits on a pixel centre, rim points on the half-pixel lattice (so edges run
    through pixel centres), every wedge convex; windings are flipped at random (rendering is two-sided).
    -> (X, Y int64 lattice coordinates [n_tri + 1], faces [n_tri,3], hub pixel (i, j))."""
    while True:
        ci, cj = rng.randint(W // 4, 3 * W // 4), rng.randint(H // 4, 3 * H // 4)
        ang = np.sort(rng.uniform(0, 2 * np.pi) + (np.arange(n_tri) + rng.uniform(-0.3, 0.3, n_tri)) * 2 * np.pi / n_tri)
        rad = rng.uniform(1.5, min(H, W) / 3, n_tri)
        rx = np.rint((ci + 0.5 + rad * np.cos(ang)) * 2).astype(I64) * 128           # multiples of half a pixel
        ry = np.rint((cj + 0.5 + rad * np.sin(ang)) * 2).astype(I64) * 128
        hx, hy = 256 * ci + 128, 256 * cj + 128
        nx, ny = np.roll(rx, -1), np.roll(ry, -1)
        if ((rx - hx) * (ny - hy) - (ry - hy) * (nx - hx) > 0).all():                # every wedge turns the same way, none degenerate
            break
    X, Y = np.concatenate([[hx], rx]), np.concatenate([[hy], ry])
    faces = np.array([[0, 1 + k, 1 + (k + 1) % n_tri] for k in range(n_tri)], I64)
    flip = rng.rand(n_tri) < 0.5
    faces[flip] = faces[flip][:, [0, 2, 1]]
    roll = rng.randint(0, 3, n_tri)
    faces = np.stack([np.roll(f, r) for f, r in zip(faces, roll)])
    return X, Y, faces, (ci, cj)


# ---- the sphere-shell bounds ------------------------------------------------------------------------------------------------------------
def index_triangles(tris):
    """Triangle soup [T,3,3] -> (verts [V,3], faces [T,3]) with equal corners merged."""
    verts, inverse = np.unique(np.asarray(tris, F32).reshape(-1, 3), axis=0, return_inverse=True)
    return verts, inverse.reshape(-1, 3).astype(np.int32)


def shell_check(face, depth, pose, intr, centre, radius, pitch, label=""):
    """The derived bounds of a marching-cubes mesh of |x - centre| - radius sampled at grid pitch h, seen through (pose, intr).

    Every vertex is the linear interpolation of a convex function along a grid edge, so it lies inside the sphere, and by at most
    h^2 / (8 (r - h)) (interpolation error h^2 / 8 times the second derivative, at most 1 / (r - h) on the edge); a face lies in one
    cube, so its points are at most h from a vertex: every mesh point has a radius in [sqrt((r - h^2 / (8 (r - h)))^2 - h^2), r].
    Snapping to the 1/256-pixel lattice moves a vertex by at most sqrt(2) 2^-9 pixels on the screen, i.e. by sqrt(2) 2^-9 z / f_px in
    space at its depth z <= z_max = |camera-space centre| + r, with f_px the smaller focal length in pixels: the rendered surface is a
    closed surface between the shells widened by that slack.  The fp32 budget, in units of 2^-24 of the magnitude rounded: the
    camera transform rounds 6 times quantities of at most z_max, and the screen coordinates 4 times (product, quotient, sum, times
    256) quantities of at most max(W, H) pixels, again z_max / f_px in space: w = slack + 2^-24 (6 z_max + 4 max(W, H) z_max / f_px).
    The depth itself rounds 10 times (two conversions and a quotient per b_k, q_k, two sums, the reciprocal -- the three b_k and
    q_k round in parallel): a relative 10 x 2^-24.

    A pixel ray that hits the sphere of radius r_in - w must be covered, at a depth between the entry depths of the spheres of radius
    r + w and r_in - w; a ray that misses the sphere of radius r + w must be a miss; the pixels in between are undecided.
    -> (hit count, miss count, undecided count, violations)."""
    H, W = face.shape
    P, K = np.asarray(pose, np.float64), np.asarray(intr, np.float64)
    C = P[:, :3] @ np.asarray(centre, np.float64) + P[:, 3]
    h, r = float(pitch), float(radius)
    r_in = np.sqrt((r - h * h / (8 * (r - h))) ** 2 - h * h)
    z_max, f_px = np.linalg.norm(C) + r, min(K[0, 0], K[1, 1])
    w = np.sqrt(2) * 2.0 ** -9 * z_max / f_px + 2.0 ** -24 * (6 * z_max + 4 * max(W, H) * z_max / f_px)
    j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.stack([(i + 0.5 - K[0, 2]) / K[0, 0], (j + 0.5 - K[1, 2]) / K[1, 1], np.ones((H, W))], axis=-1)
    dd, dC, CC = (d * d).sum(-1), d @ C, C @ C

    def entry(R):
        disc = dC * dC - dd * (CC - R * R)
        return disc, (dC - np.sqrt(np.maximum(disc, 0))) / dd
    disc_in, z_in = entry(r_in - w)
    disc_out, z_out = entry(r + w)
    hit, miss = disc_in > 0, disc_out < 0
    tol = 10 * 2.0 ** -24
    bad = (hit & ((face < 0) | (depth < z_out * (1 - tol)) | (depth > z_in * (1 + tol)))) | (miss & (face >= 0))
    undecided = int((~hit & ~miss).sum())
    print("shell check %s %dx%d: %d hit, %d miss, %d undecided, %d violations (r_in %.5f, w %.2e)"
          % (label, H, W, hit.sum(), miss.sum(), undecided, bad.sum(), r_in, w))
    return int(hit.sum()), int(miss.sum()), undecided, int(bad.sum())


SHELL_VIEWS = ((32, 32, 5.0, look_pose(0.7, -0.4, 5.0, 0.2)), (20, 33, 4.3, look_pose(-2.1, 0.6, 4.3, -1.0)))       # H, W, distance, pose
SHELL_SPHERE = dict(S=16, radius=0.3, centre=(0.02, -0.03, 0.01))
