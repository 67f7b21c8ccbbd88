"""Numpy restatement of the dual contouring of include/shapeclipper_hip.h (csrc/dual_contour.hip, ops.dual_contour_mesh), written from
the header's text, and the grids its tests run on.  Pure-Python loops over the surface cells: small grids only.

  dual_contour(level, normals, iso, reg)              every operation of the cell solve one fp32 operation, in the header's order; the GPU
                                                      tests compare bits against it
  dual_contour(level, normals, iso, reg, exact=True)  the same regularised system summed in float64 and solved by numpy.linalg.solve

Measured on the CPU over all grids of `grids()` (tests/test_dual_contour_host.py prints it): the largest absolute difference of a
vertex coordinate between the two is 1.12315882e-06 grid units (on the torus; coordinates reach 15, where one fp32 ulp is 9.5e-07) --
the host test allows 8 times that, FP32_VS_EXACT_BOUND, because a 3 x 3 solve has no wider spread of conditioning than these grids show.
"""
import numpy as np

f32 = np.float32
EDGES = ((0, 1), (0, 2), (0, 4), (1, 3), (1, 5), (2, 3), (2, 6), (3, 7), (4, 5), (4, 6), (5, 7), (6, 7))
FLT_MAX = f32(3.402823466e+38)
FP32_VS_EXACT_BOUND = 8 * 1.12315882e-06


def crossings(level, iso=0.0):
    """level [S,S,S] -> (verts [V,3] fp32, vmap {(x, y, z, axis): vertex number}): the vertices of the indexed marching-cubes mesh, one
    per grid edge (p, p + e_axis) whose ends lie on different sides of iso (inside = value < iso), ordered by the linear index of p,
    then axis, at the soup's interpolation a_j + t (b_j - a_j) of ALL three coordinates, t = (iso - f(a)) / (f(b) - f(a)) from the lower
    end a to the upper end b (csrc/isosurface.hip, iso_vertex_ab): a NaN t, from a NaN level value, makes every coordinate NaN."""
    level = np.asarray(level, dtype=f32)
    S = level.shape[0]
    iso = f32(iso)
    verts, vmap = [], {}
    with np.errstate(all="ignore"):
        for x in range(S):
            for y in range(S):
                for z in range(S):
                    fa = level[x, y, z]
                    for axis in range(3):
                        q = [x, y, z]
                        q[axis] += 1
                        if q[axis] >= S:
                            continue
                        fb = level[tuple(q)]
                        if bool(fa < iso) == bool(fb < iso):
                            continue
                        t = f32(iso - fa) / f32(fb - fa)
                        vmap[(x, y, z, axis)] = len(verts)
                        verts.append([f32(a) + t * f32(b - a) for a, b in zip((x, y, z), q)])
    return np.asarray(verts, dtype=f32).reshape(-1, 3), vmap


def solve_cell_fp32(g, P, N, reg):
    """g: the cell's lower corner (3 ints); P, N: its crossings and their normals in edge order (lists of 3-vectors of fp32) -> x (3 fp32)."""
    with np.errstate(all="ignore"):
        k = len(P)
        s = [f32(0.0)] * 3
        for p in P:
            s = [s[j] + f32(p[j]) for j in range(3)]
        kf = f32(k)
        c = [s[j] / kf for j in range(3)]
        a00 = a01 = a02 = a11 = a12 = a22 = f32(0.0)
        b = [f32(0.0)] * 3
        for p, n in zip(P, N):
            n = [f32(v) for v in n]
            if not all(abs(v) <= FLT_MAX for v in n):
                continue
            d = [f32(p[j]) - c[j] for j in range(3)]
            w = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2]
            a00 = a00 + n[0] * n[0]; a01 = a01 + n[0] * n[1]; a02 = a02 + n[0] * n[2]
            a11 = a11 + n[1] * n[1]; a12 = a12 + n[1] * n[2]; a22 = a22 + n[2] * n[2]
            b = [b[j] + n[j] * w for j in range(3)]
        r = f32(reg) * kf
        a00 = a00 + r; a11 = a11 + r; a22 = a22 + r
        l10 = a01 / a00
        l20 = a02 / a00
        e1 = a11 - l10 * a01
        t21 = a12 - l20 * a01
        l21 = t21 / e1
        e2 = (a22 - l20 * a02) - l21 * t21
        z1 = b[1] - l10 * b[0]
        z2 = (b[2] - l20 * b[0]) - l21 * z1
        y2 = z2 / e2
        y1 = z1 / e1 - l21 * y2
        y0 = (b[0] / a00 - l10 * y1) - l20 * y2
        x = [c[0] + y0, c[1] + y1, c[2] + y2]
        for j in range(3):
            assert type(x[j]) is np.float32                      # nothing above left fp32
            if not x[j] >= f32(g[j]):
                x[j] = f32(g[j])
            if not x[j] <= f32(g[j] + 1):
                x[j] = f32(g[j] + 1)
        return x


def solve_cell_exact(g, P, N, reg):
    """The same system in float64: (sum n n^T + reg k I) y = sum n (n . (p - c)) by numpy.linalg.solve, x = c + y, clamped."""
    with np.errstate(all="ignore"):
        P64 = np.asarray(P, dtype=np.float64).reshape(-1, 3)
        k = len(P64)
        c = P64.sum(0) / k
        A, b = reg * k * np.eye(3), np.zeros(3)
        for p, n in zip(P64, np.asarray(N, dtype=np.float64).reshape(-1, 3)):
            if not np.isfinite(n).all():
                continue
            A += np.outer(n, n)
            b += n * (n @ (p - c))
        x = c + (np.linalg.solve(A, b) if np.isfinite(A).all() and np.isfinite(b).all() else np.full(3, np.nan))
        for j in range(3):
            if not x[j] >= g[j]:
                x[j] = g[j]
            if not x[j] <= g[j] + 1:
                x[j] = g[j] + 1
        return list(x)


def dual_contour(level, normals, iso=0.0, reg=0.05, exact=False):
    """level [S,S,S], normals [V,3] (one per vertex of crossings(level, iso)) -> (verts [Vd,3], faces [Fd,3] int32) of ONE image; verts
    fp32, or float64 with exact=True."""
    level = np.asarray(level, dtype=f32)
    normals = np.asarray(normals, dtype=f32).reshape(-1, 3)
    S = level.shape[0]
    pv, vmap = crossings(level, iso)
    assert normals.shape[0] == pv.shape[0]
    inside = level < f32(iso)
    corner = lambda g, v: (g[0] + (v & 1), g[1] + ((v >> 1) & 1), g[2] + ((v >> 2) & 1))
    solve = solve_cell_exact if exact else solve_cell_fp32
    verts, cell = [], {}
    for x in range(S - 1):
        for y in range(S - 1):
            for z in range(S - 1):
                g = (x, y, z)
                ins = [bool(inside[corner(g, v)]) for v in range(8)]
                if all(ins) or not any(ins):
                    continue
                P, N = [], []
                for ca, cb in EDGES:
                    if ins[ca] != ins[cb]:
                        v = vmap[corner(g, ca) + ((cb - ca) >> 1,)]
                        P.append(pv[v]); N.append(normals[v])
                cell[g] = len(verts)
                verts.append(solve(g, P, N, reg))
    faces = []
    for x in range(S - 1):
        for y in range(S - 1):
            for z in range(S - 1):
                P = (x, y, z)
                for a in range(3):
                    b, c = (a + 1) % 3, (a + 2) % 3
                    Q = list(P); Q[a] += 1
                    if inside[P] == inside[tuple(Q)] or not (1 <= P[b] <= S - 2 and 1 <= P[c] <= S - 2):
                        continue
                    q = []
                    for db, dc in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
                        C = list(P); C[b] += db; C[c] += dc
                        q.append(cell[tuple(C)])
                    faces += [(q[0], q[1], q[2]), (q[0], q[2], q[3])] if inside[P] else [(q[0], q[2], q[1]), (q[0], q[3], q[2])]
    return (np.asarray(verts, dtype=np.float64 if exact else f32).reshape(-1, 3), np.asarray(faces, dtype=np.int32).reshape(-1, 3))


# ---- grids ---------------------------------------------------------------------------------------------------------------------------
def _axes(S):
    ax = np.linspace(-1, 1, S)
    return np.meshgrid(ax, ax, ax, indexing="ij")


def _world(pv, S):
    return pv.astype(np.float64) * (2.0 / (S - 1)) - 1.0


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


def sphere(S=16, r=0.55, centre=(0.1, -0.05, 0.2)):
    """(level, analytic unit normals at the crossing vertices)"""
    X, Y, Z = _axes(S)
    level = (np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) - r).astype(f32)
    return level, _unit(_world(crossings(level)[0], S) - np.asarray(centre))


def torus(S=16, R=0.55, r=0.27):
    X, Y, Z = _axes(S)
    level = (np.sqrt((np.sqrt(X * X + Y * Y) - R) ** 2 + Z * Z) - r).astype(f32)
    w = _world(crossings(level)[0], S)
    rho = np.sqrt(w[:, 0] ** 2 + w[:, 1] ** 2)
    return level, _unit(np.stack([w[:, 0] * (rho - R) / rho, w[:, 1] * (rho - R) / rho, w[:, 2]], 1))


def finite_difference_normals(level, iso=0.0):
    """Unit normals at the crossing vertices from numpy.gradient of the grid, interpolated linearly along each crossing edge."""
    level = np.asarray(level, dtype=f32)
    grad = np.stack(np.gradient(level.astype(np.float64)), -1)
    pv, vmap = crossings(level, iso)
    out = np.zeros((len(pv), 3))
    for (x, y, z, axis), v in vmap.items():
        q = [x, y, z]; q[axis] += 1
        t = float(pv[v][axis]) - (x, y, z)[axis]
        out[v] = (1 - t) * grad[x, y, z] + t * grad[tuple(q)]
    with np.errstate(all="ignore"):
        return _unit(out)


def smooth_noise(S=9, seed=0):
    """A seeded smooth random field: a few low-frequency waves (the surface meets the faces of the grid: an open mesh)."""
    rng = np.random.RandomState(seed)
    X, Y, Z = _axes(S)
    level = np.zeros((S, S, S))
    for _ in range(6):
        k, ph = rng.uniform(-3, 3, 3), rng.uniform(0, 2 * np.pi)
        level += rng.uniform(0.3, 1.0) * np.sin(k[0] * X + k[1] * Y + k[2] * Z + ph)
    level = level.astype(f32)
    return level, finite_difference_normals(level)


def with_nans(S=9, seed=3):
    """A noise grid with one NaN level value and one NaN normal.  The NaN replaces the first interior outside value whose +x neighbour is
    inside, so it stays outside, the edge between the two still crosses and its vertex is NaN; numpy.gradient spreads NaN to the
    normals of the crossings around it.  The NaN normal sits at the last vertex whose normal was finite, away from all that."""
    level, _ = smooth_noise(S, seed)
    level = level.copy()
    x, y, z = next((x, y, z) for x in range(1, S - 2) for y in range(1, S - 1) for z in range(1, S - 1)
                   if not level[x, y, z] < 0 and level[x + 1, y, z] < 0)
    level[x, y, z] = np.nan
    normals = finite_difference_normals(level)
    normals[np.flatnonzero(np.isfinite(normals).all(1))[-1], 1] = np.nan
    return level, normals


def box(S=12, lo=2.5, hi=8.5):
    """The exact SDF of the box [lo, hi]^3 in grid-index units; normals are the axis unit vectors of the crossed face (a crossing edge
    along axis a crosses a face perpendicular to a: the normal is -e_a at lo, +e_a at hi)."""
    g = np.arange(S, dtype=np.float64)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    c, h = (lo + hi) / 2, (hi - lo) / 2
    q = np.stack([np.abs(X - c) - h, np.abs(Y - c) - h, np.abs(Z - c) - h], -1)
    level = (np.linalg.norm(np.maximum(q, 0), axis=-1) + np.minimum(q.max(-1), 0)).astype(f32)
    pv, vmap = crossings(level)
    normals = np.zeros((len(pv), 3), f32)
    for (x, y, z, axis), v in vmap.items():
        normals[v, axis] = -1.0 if pv[v][axis] < c else 1.0
    return level, normals


def tiny(S, seed):
    """S = 2 or 3: random values, random unit normals."""
    rng = np.random.RandomState(seed)
    level = rng.randn(S, S, S).astype(f32)
    return level, _unit(rng.randn(len(crossings(level)[0]), 3))


def grids():
    """{name: (level [S,S,S] fp32, normals [V,3] fp32)}: every grid the bit-for-bit tests run on."""
    out = {"sphere": sphere(), "torus": torus(), "nans": with_nans(), "box": box(), "s2": tiny(2, 11), "s3": tiny(3, 12),
           "outside": (np.full((9, 9, 9), 1.0, f32), np.zeros((0, 3), f32))}
    for seed in range(3):
        out["noise%d" % seed] = smooth_noise(9, seed)
    return out
