"""numpy restatement of sc_level_ambient_occlusion (include/shapeclipper_hip.h): ops.level_ambient_occlusion one rounding at a time --
the folded direction and its weight, the sample positions, the empty-cell rule, the z-y-x trilinear value, the pairwise sums.  numpy's
elementwise float32 operations round once each and never fuse, which is what the kernel is built to do.  Also the directions, the
quadrature error of the 64 directions, and the level grids that the host and GPU tests share."""
import math
import os
import sys

import numpy as np

DIRS = 64               # SC_LEVEL_AO_DIRS
MAX_STEPS = 4096        # SC_LEVEL_AO_MAX_STEPS
F32 = np.float32


def directions():
    """The Fibonacci set of ops.ao_directions, restated: [64,3] float32 from float64."""
    k = np.arange(DIRS, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / DIRS
    r = np.sqrt(1.0 - z * z)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(F32)


def step_count(radius, step):
    return int(math.ceil(radius / step))


def tree_sum(a):
    """[N,64] float32 -> [N]: a[j+1][k] = a[j][2k] + a[j][2k+1]."""
    a = np.asarray(a, F32)
    while a.shape[1] > 1:
        a = a[:, 0::2] + a[:, 1::2]
    return a[:, 0]


def ambient_occlusion(level, points, normals, image, radius, step=0.5, bias=1.0, iso=0.0, dirs=None):
    """level [B,S,S,S], points [N,3], normals [N,3], image [N] -> (ao [N] float32, mask [N] int64).  ValueError("bad_image") where the
    kernel sets its flag."""
    level = np.asarray(level, F32)
    B, S = level.shape[0], level.shape[1]
    assert level.shape == (B, S, S, S) and 2 <= S <= 1024
    p = np.asarray(points, F32).reshape(-1, 3)
    n = np.asarray(normals, F32).reshape(-1, 3)
    image = np.asarray(image, np.int64).reshape(-1)
    N = len(p)
    M = step_count(radius, step)
    assert 1 <= M <= MAX_STEPS
    step, bias, iso = F32(step), F32(bias), F32(iso)
    D = directions() if dirs is None else np.asarray(dirs, F32)
    if ((image < 0) | (image >= B)).any():
        raise ValueError("bad_image")
    top = F32(S - 1)
    with np.errstate(all="ignore"):
        finite = np.isfinite(p).all(axis=1) & np.isfinite(n).all(axis=1)
        dn = (D[None, :, 0] * n[:, None, 0] + D[None, :, 1] * n[:, None, 1]) + D[None, :, 2] * n[:, None, 2]      # [N,64]
        d = np.where((dn < 0)[..., None], -D[None], D[None])                                                    # [N,64,3]
        w = np.where(finite[:, None], np.abs(dn), F32(0))
        p0 = p + bias * n
        alive = np.broadcast_to(finite[:, None], (N, DIRS)).copy()          # rays still marching
        is_open = np.ones((N, DIRS), bool)
        for s in range(1, M + 1):
            if not alive.any():
                break
            t = F32(s) * step
            rows, lanes = np.nonzero(alive)
            q = p0[rows] + t * d[rows, lanes]                               # [R,3]
            inside = ((q >= 0) & (q <= top)).all(axis=1)
            alive[rows[~inside], lanes[~inside]] = False                    # OPEN
            rows, lanes, q = rows[inside], lanes[inside], q[inside]
            i = np.minimum(np.floor(q).astype(np.int64), S - 2)
            f = q - i.astype(F32)
            b = image[rows]
            v = np.stack([level[b, i[:, 0] + a0, i[:, 1] + a1, i[:, 2] + a2] for a0 in (0, 1) for a1 in (0, 1) for a2 in (0, 1)],
                         axis=1).reshape(-1, 2, 2, 2)
            occupied = (v < iso).reshape(-1, 8).any(axis=1)
            fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
            u = v[..., 0] + fz[:, None, None] * (v[..., 1] - v[..., 0])     # along z: [R,2,2]
            u = u[..., 0] + fy[:, None] * (u[..., 1] - u[..., 0])           # along y: [R,2]
            val = u[:, 0] + fx * (u[:, 1] - u[:, 0])                        # along x
            closed = occupied & (val < iso)
            is_open[rows[closed], lanes[closed]] = False
            alive[rows[closed], lanes[closed]] = False
        W = tree_sum(w)
        V = tree_sum(np.where(is_open, w, F32(0)))
        ok = W > 0
        ao = np.where(ok, V / np.where(ok, W, F32(1)), F32(1)).astype(F32)
    bits = (is_open.astype(np.uint64) << np.arange(DIRS, dtype=np.uint64)[None]).sum(axis=1, dtype=np.uint64)
    mask = np.where(ok, bits, np.uint64(0xFFFFFFFFFFFFFFFF)).astype(np.uint64).view(np.int64)
    return ao, mask


def cell_bits(level, iso=0.0):
    """The bit volume of the kernel's first launch as booleans [B,S-1,S-1,S-1]: a cell is occupied when one of its 8 corners is < iso."""
    below = np.asarray(level, F32) < F32(iso)
    out = np.zeros(tuple(np.array(below.shape) - [0, 1, 1, 1]), bool)
    for a0 in (0, 1):
        for a1 in (0, 1):
            for a2 in (0, 1):
                out |= below[:, a0:below.shape[1] - 1 + a0, a1:below.shape[2] - 1 + a1, a2:below.shape[3] - 1 + a2]
    return out


def popcount(mask):
    return np.array([bin(int(m) & 0xFFFFFFFFFFFFFFFF).count("1") for m in np.asarray(mask).reshape(-1)])


def half_space_error(trials=1000, seed=0):
    """The quadrature error of the 64 directions: for `trials` random unit normals n and a random m perpendicular to n, the |D . n|-
    weighted share of the folded directions with d . m >= 0 against the exact 0.5 (a wall through the point, at right angles to the
    surface).  -> the errors [trials] float64."""
    rng = np.random.default_rng(seed)
    D = directions().astype(np.float64)
    n = rng.normal(size=(trials, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    m = np.cross(n, rng.normal(size=(trials, 3)))
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    dn = n @ D.T                                                            # [T,64]
    side = (m @ D.T) * np.sign(dn)
    w = np.abs(dn)
    return (np.where(side >= 0, w, 0.0).sum(axis=1) / w.sum(axis=1)) - 0.5


# ---- the shapes: level grids (negative inside the solid), and surface points with normals ------------------------------------------------
def _axes(S):
    g = np.arange(S, dtype=np.float64)
    return np.meshgrid(g, g, g, indexing="ij")


def sphere_level(S=17, centre=(8.0, 8.0, 8.0), r=5.3):
    x, y, z = _axes(S)
    return (np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - r).astype(F32)


def box_level(S=17, centre=(8.0, 8.0, 8.0), half=4.4):
    x, y, z = _axes(S)
    return (np.maximum(np.maximum(np.abs(x - centre[0]), np.abs(y - centre[1])), np.abs(z - centre[2])) - half).astype(F32)


def crease_level(S=33, at=8.0):
    """A floor below z = at and a wall behind x = at: level = min(z - at, x - at)."""
    x, _, z = _axes(S)
    return np.minimum(z - at, x - at).astype(F32)


TWO_SPHERES = ((4.5, 8.0, 8.0), (12.5, 8.0, 8.0), 3.0)


def two_spheres_level(S=17):
    c1, c2, r = TWO_SPHERES
    return np.minimum(sphere_level(S, c1, r), sphere_level(S, c2, r))


PIT = dict(top=8.0, bottom=3.0, centre=8.0, half=2.0)


def pit_level(S=17):
    """The solid below z = top with a square shaft of side 2 half down to z = bottom."""
    x, y, z = _axes(S)
    shaft = np.maximum(np.maximum(np.abs(x - PIT["centre"]), np.abs(y - PIT["centre"])) - PIT["half"], PIT["bottom"] - z)
    return np.maximum(z - PIT["top"], -shaft).astype(F32)


_MESH = {}


def mc_vertices(name, level):
    """The distinct marching-cubes vertices (grid-index units, [V,3] float32) of a level grid, by oracle/isosurface_ref; once per name."""
    if name not in _MESH:
        root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
        if root not in sys.path:
            sys.path.insert(0, root)
        from oracle import isosurface_ref
        tris = np.ascontiguousarray(isosurface_ref.marching_cubes(level), F32).reshape(-1, 3)
        _MESH[name] = np.unique(tris, axis=0).astype(F32)
    return _MESH[name]


def sphere_normals(verts, centre):
    d = verts.astype(np.float64) - np.asarray(centre, np.float64)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)


def box_normals(verts, centre):
    """A subgradient of the max-norm at every vertex: the unit vector of the axis of largest |offset|."""
    d = verts.astype(np.float64) - np.asarray(centre, np.float64)
    k = np.abs(d).argmax(axis=1)
    out = np.zeros_like(d)
    out[np.arange(len(d)), k] = np.sign(d[np.arange(len(d)), k])
    return out.astype(F32)
