"""Numpy restatement of the point-to-mesh distance of include/shapeclipper_hip.h (csrc/point_mesh.hip, ops.point_mesh_distance),
written from the header's text, and the meshes and queries its tests run on.

  pair(p, a, b, c)                  the closest point of every (point, triangle) pair, every operation one fp32 operation in the
                                    header's order (numpy rounds each array operation once); the GPU tests compare bits against it
  pair(p, a, b, c, dtype=float64)   the same walk in float64
  brute(points, verts, faces)       the minimum over one image's valid faces with the tie rule, fp32 or float64
  point_mesh(points, verts, faces, v_count, f_count)   the packed, batched form of the entry points

  exact_distance2 / brute_exact     float64 by another route (segments and plane), the yardstick of the fp32 arithmetic

Measured on the CPU (tests/test_point_mesh_host.py prints the figures) over `cases()`, the inputs of the GPU tests, as the largest
|sqrt(d fp32) - sqrt(d float64)| of a query's minimum, the float64 side being brute_exact, never the kernel:
  * meshes of ordinary triangles (sphere, batch3, huge, flat, n1, n65, f1; vertices within +-0.7, queries up to 9 away): 5.35e-07, on
    the sphere's far queries, where one fp32 ulp of the distance is 4.8e-07; 1.7e-07 among queries within 0.3 of the mesh;
  * the degenerate mesh (duplicates, point triangles, collinear triangles and slivers of width 1e-6): 1.16e-06, the slivers' own
    width -- a triangle whose sin^2 at a is below FLAT is taken as its edges.  (Without that rule the figure was 1.6e-03: on a
    triangle of almost no area the interior weights vb / den, vc / den are quotients of rounding noise, and the float64 twin of the
    walk was itself off by 2.6e-03 on the exactly collinear ones.)
The host test allows 4 times each figure (FP32_VS_EXACT_BOUND, FP32_VS_EXACT_BOUND_DEGENERATE) for other seeds.
"""
import numpy as np

f32 = np.float32
FLAT = 1.0e-5                   # the interior region needs sin^2 of the angle at a above this: thinner triangles count as their edges
FP32_VS_EXACT_BOUND = 4 * 5.35e-07
FP32_VS_EXACT_BOUND_DEGENERATE = 4 * 1.16e-06


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _segment(p, s, e):
    """Clamped closest point of the segment s + t e: (q, d)."""
    zero, one = p.dtype.type(0), p.dtype.type(1)
    l = _dot(e, e)
    t = _dot(p - s, e) / l
    t = np.where(l > zero, t, zero)
    t = np.where(t >= zero, t, zero)
    t = np.where(t > one, one, t)
    q = s + t[..., None] * e
    r = p - q
    return q, _dot(r, r)


def pair(p, a, b, c, dtype=f32):
    """p [..., 3] against triangles a, b, c [..., 3] (broadcast against each other) -> (d [...], q [..., 3], region [...]): the header's
    "Arithmetic of one pair".  region: 0 A, 1 B, 2 AB, 3 C, 4 AC, 5 BC, 6 interior, 7 the segment fallback."""
    p, a, b, c = (np.asarray(x, dtype=dtype) for x in (p, a, b, c))
    p, a, b, c = np.broadcast_arrays(p, a, b, c)
    zero = dtype(0)
    with np.errstate(all="ignore"):
        ab, ac, bc = b - a, c - a, c - b
        ap, bp, cp = p - a, p - b, p - c
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e1, e2 = d4 - d3, d5 - d6
        nab, nac, nbc = d1 - d3, d2 - d6, e1 + e2
        den = (va + vb) + vc
        tests = [
            (d1 <= zero) & (d2 <= zero),
            (d3 >= zero) & (d4 <= d3),
            (vc <= zero) & (d1 >= zero) & (d3 <= zero) & (nab > zero),
            (d6 >= zero) & (d5 <= d6),
            (vb <= zero) & (d2 >= zero) & (d6 <= zero) & (nac > zero),
            (va <= zero) & (e1 >= zero) & (e2 >= zero) & (nbc > zero),
            (den > zero) & (va >= zero) & (vb >= zero) & (vc >= zero) & (den > dtype(FLAT) * (_dot(ab, ab) * _dot(ac, ac))),
        ]
        v, w = vb / den, vc / den
        points = [
            a, b, a + (d1 / nab)[..., None] * ab, c, a + (d2 / nac)[..., None] * ac, b + (e1 / nbc)[..., None] * bc,
            (a + v[..., None] * ab) + w[..., None] * ac,
        ]
        # the fallback: AB's candidate first, AC's and BC's replace it when strictly smaller
        q, d = _segment(p, a, ab)
        for s, e in ((a, ac), (b, bc)):
            q2, dd = _segment(p, s, e)
            better = dd < d
            d = np.where(better, dd, d)
            q = np.where(better[..., None], q2, q)
        region = np.full(d.shape, 7, dtype=np.int8)
        for k in range(6, -1, -1):                      # the FIRST test that holds wins: apply them last to first
            r = p - points[k]
            d = np.where(tests[k], _dot(r, r), d)
            q = np.where(tests[k][..., None], points[k], q)
            region = np.where(tests[k], np.int8(k), region)
    return d, q, region


def brute(points, verts, faces, dtype=f32, chunk=256):
    """points [N,3], verts [V,3], faces [F,3] (indices into verts) of ONE image -> (dist2 [N], face [N] int32, closest [N,3]): the winner
    of  d < best || (d == best && f < best_f)  over the faces whose indices lie in [0, V), i.e. the lowest face among the exact minima;
    NaN never wins.  No winner: +Inf, -1, 0.  A query that is not finite: NaN, -1, NaN."""
    points = np.asarray(points, dtype=dtype).reshape(-1, 3)
    verts = np.asarray(verts, dtype=dtype).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    N, V = len(points), len(verts)
    dist2 = np.full(N, np.inf, dtype=dtype)
    face = np.full(N, -1, dtype=np.int32)
    closest = np.zeros((N, 3), dtype=dtype)
    ok = ((faces >= 0) & (faces < V)).all(axis=1)
    keep = np.nonzero(ok)[0]
    if len(keep):
        a, b, c = (verts[faces[keep, k]][None] for k in range(3))
        for s in range(0, N, chunk):
            p = points[s:s + chunk, None, :]
            d, q, _ = pair(p, a, b, c, dtype)
            comparable = ~np.isnan(d)
            any_ok = comparable.any(axis=1)
            dm = np.where(comparable, d, np.inf)
            m = dm.min(axis=1)
            first = np.argmax(comparable & (dm == m[:, None]), axis=1)      # the first (lowest) face attaining the minimum
            rows = np.arange(len(m))
            dist2[s:s + chunk] = np.where(any_ok, m, np.inf)
            face[s:s + chunk] = np.where(any_ok, keep[first], -1)
            closest[s:s + chunk] = np.where(any_ok[:, None], q[rows, first], 0)
    bad = ~np.isfinite(points).all(axis=1)
    dist2[bad], face[bad], closest[bad] = np.nan, -1, np.nan
    return dist2, face, closest


def exact_distance2(p, a, b, c):
    """Float64 squared distance from p to triangle (a, b, c) by another route than the walk, robust on triangles of (almost) no area,
    where the walk's interior weights are quotients of rounding noise in float64 too: the minimum over the three clamped segments, and
    the distance to the plane when the triangle has a plane (sin of its angle at a above 1e-10) and p projects inside it."""
    p, a, b, c = (np.asarray(x, dtype=np.float64) for x in (p, a, b, c))
    p, a, b, c = np.broadcast_arrays(p, a, b, c)
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d = np.minimum(np.minimum(_segment(p, a, ab)[1], _segment(p, a, ac)[1]), _segment(p, b, c - b)[1])
        n = np.cross(ab, ac)
        nn = _dot(n, n)
        solid = nn > 1e-20 * _dot(ab, ab) * _dot(ac, ac)
        v = _dot(np.cross(ap, ac), n) / nn
        w = _dot(np.cross(ab, ap), n) / nn
        inside = solid & (v >= 0) & (w >= 0) & (v + w <= 1)
        return np.where(inside, np.minimum(_dot(ap, n) ** 2 / nn, d), d)


def brute_exact(points, verts, faces, v_count, f_count, chunk=256):
    """The float64 brute force the fp32 arithmetic is held to: dist2 [B,N] float64 = the minimum of exact_distance2 over the valid faces
    of the query's image (+Inf without one)."""
    points = np.asarray(points, dtype=np.float64)
    out = np.full(points.shape[:2], np.inf)
    v0 = f0 = 0
    for i in range(points.shape[0]):
        v = np.asarray(verts[v0:v0 + v_count[i]], dtype=np.float64)
        f = np.asarray(faces[f0:f0 + f_count[i]], dtype=np.int64)
        f = f[((f >= 0) & (f < len(v))).all(axis=1)]
        if len(f):
            for s in range(0, points.shape[1], chunk):
                out[i, s:s + chunk] = exact_distance2(points[i, s:s + chunk, None, :], v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]).min(axis=1)
        v0, f0 = v0 + int(v_count[i]), f0 + int(f_count[i])
    return out


def point_mesh(points, verts, faces, v_count, f_count, dtype=f32):
    """The entry points' packed form: points [B,N,3], verts [Vtot,3], faces [Ftot,3] local to each image's slice -> (dist2 [B,N],
    face [B,N], closest [B,N,3])."""
    points = np.asarray(points)
    out = [], [], []
    v0 = f0 = 0
    for b in range(points.shape[0]):
        res = brute(points[b], verts[v0:v0 + v_count[b]], faces[f0:f0 + f_count[b]], dtype)
        for o, r in zip(out, res):
            o.append(r)
        v0, f0 = v0 + int(v_count[b]), f0 + int(f_count[b])
    return tuple(np.stack(o) for o in out)


def pack(meshes):
    """[(verts [V,3], faces [F,3])] -> (verts [Vtot,3] fp32, faces [Ftot,3] int32, v_count [B] int32, f_count [B] int32)."""
    verts = np.concatenate([np.asarray(v, dtype=f32).reshape(-1, 3) for v, _ in meshes])
    faces = np.concatenate([np.asarray(f, dtype=np.int32).reshape(-1, 3) for _, f in meshes])
    return (verts, faces, np.asarray([len(np.asarray(v).reshape(-1, 3)) for v, _ in meshes], dtype=np.int32),
            np.asarray([len(np.asarray(f).reshape(-1, 3)) for _, f in meshes], dtype=np.int32))


# ---- the meshes and queries of the tests -------------------------------------------------------------------------------------------------
def index_soup(tris):
    """triangles [T,3,3] -> (verts [V,3] fp32, faces [T,3] int32): vertices with the same bits become one."""
    tris = np.ascontiguousarray(np.asarray(tris, dtype=f32).reshape(-1, 3))
    _, first, inverse = np.unique(tris.view(np.uint32), axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first)                           # vertices in order of first appearance
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    return tris[first[order]], rank[inverse.reshape(-1)].reshape(-1, 3).astype(np.int32)


_SPHERE = {}


def sphere_mesh(S=16, r=0.55, centre=(0.1, -0.05, 0.2)):
    """The marching-cubes mesh (oracle/isosurface_ref.py, the kernels' vertex set) of the sphere of tests/dual_contour_ref.py on an S^3
    grid, indexed, rescaled from grid units to [-0.6, 0.6]: a few hundred triangles."""
    key = (S, r, tuple(centre))
    if key not in _SPHERE:
        import dual_contour_ref
        from oracle import isosurface_ref
        level, _ = dual_contour_ref.sphere(S, r, centre)
        verts, faces = index_soup(isosurface_ref.marching_cubes(level, 0.0))
        _SPHERE[key] = ((verts / f32(S) * f32(1.2) - f32(0.6)).astype(f32), faces)
    v, f = _SPHERE[key]
    return v.copy(), f.copy()


def sphere_queries(verts, faces, n=2000, seed=0):
    """n queries for a mesh: a fifth each of points in its bounding box (inside and outside the surface), points just outside the box,
    points far away (several box sizes: the walk gives up on them), copies of mesh vertices, and edge midpoints."""
    rng = np.random.RandomState(seed)
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    k = n // 5
    box = rng.uniform(lo, hi, (k, 3))
    near = rng.uniform(lo - 0.1, hi + 0.1, (k, 3))
    far = rng.uniform(-1, 1, (k, 3))
    far = far / np.linalg.norm(far, axis=1, keepdims=True) * rng.uniform(3, 9, (k, 1))
    at_verts = verts[rng.randint(0, len(verts), k)]
    e = faces[rng.randint(0, len(faces), n - 4 * k)]
    mid = (verts[e[:, 0]] + verts[e[:, 1]]) * f32(0.5)
    return np.concatenate([box, near, far, at_verts, mid]).astype(f32)


def tiny_triangles(seed, n, spread=0.6, size=0.01):
    """n small random triangles with vertices within about +-spread: (verts [3n,3], faces [n,3]), no shared vertices."""
    rng = np.random.RandomState(seed)
    centre = rng.uniform(-spread, spread, (n, 1, 3))
    verts = (centre + rng.uniform(-size, size, (n, 3, 3))).astype(f32).reshape(-1, 3)
    return verts, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def huge_among_tiny(seed=3, n=500):
    """One triangle across the whole box (face 0) among n tiny ones: the large list."""
    verts, faces = tiny_triangles(seed, n)
    big = np.asarray([[-0.7, -0.7, -0.65], [0.7, -0.6, 0.7], [-0.5, 0.7, 0.6]], dtype=f32)
    return np.concatenate([big, verts]), np.concatenate([np.asarray([[0, 1, 2]], dtype=np.int32), faces + 3])


def degenerate_mesh(seed=5):
    """50 exact duplicates of one triangle (faces 0..49), 20 point triangles (a == b == c), 40 collinear triangles and 40 slivers, among
    100 tiny ordinary ones."""
    rng = np.random.RandomState(seed)
    tri = np.asarray([[0.1, 0.0, 0.05], [0.4, 0.1, 0.0], [0.2, 0.35, 0.1]], dtype=f32)
    verts, faces = [tri], [np.tile(np.asarray([[0, 1, 2]], dtype=np.int32), (50, 1))]
    n = 3
    pts = rng.uniform(-0.6, 0.6, (20, 3)).astype(f32)
    verts.append(pts)
    faces.append(np.repeat(np.arange(20, dtype=np.int32)[:, None], 3, axis=1) + n)
    n += 20
    a = rng.uniform(-0.6, 0.6, (80, 3)).astype(f32)
    e = rng.uniform(-0.2, 0.2, (80, 3)).astype(f32)
    t = rng.uniform(-1, 2, (80, 1)).astype(f32)
    c = a + t * e
    c[40:] += rng.uniform(-1e-6, 1e-6, (40, 3)).astype(f32)             # slivers: almost collinear
    verts.append(np.stack([a, a + e, c], axis=1).reshape(-1, 3))
    faces.append(np.arange(240, dtype=np.int32).reshape(80, 3) + n)
    n += 240
    tv, tf = tiny_triangles(seed + 1, 100)
    verts.append(tv)
    faces.append(tf + n)
    return np.concatenate(verts).astype(f32), np.concatenate(faces).astype(np.int32)


def flat_mesh(n=12):
    """An n x n grid of quads in the plane z = 0.25 (every z equal), two triangles each, shared vertices."""
    g = np.linspace(-0.5, 0.5, n + 1, dtype=f32)
    X, Y = np.meshgrid(g, g, indexing="ij")
    verts = np.stack([X, Y, np.full_like(X, 0.25)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v00 = (i * (n + 1) + j).reshape(-1)
    v10, v01, v11 = v00 + n + 1, v00 + 1, v00 + n + 2
    faces = np.concatenate([np.stack([v00, v10, v11], 1), np.stack([v00, v11, v01], 1)]).astype(np.int32)
    return verts.astype(f32), faces


def queries_around(verts, faces, n, seed):
    """n queries for any mesh: half uniform around its bounding box, a quarter copies of vertices, a quarter points drawn on the faces."""
    rng = np.random.RandomState(seed)
    lo, hi = verts.min(axis=0) - 0.15, verts.max(axis=0) + 0.15
    k = n // 4
    box = rng.uniform(lo, hi, (n - 2 * k, 3))
    at_verts = verts[rng.randint(0, len(verts), k)]
    f = faces[rng.randint(0, len(faces), k)]
    u = rng.uniform(0, 1, (k, 2))
    u = np.where(u.sum(axis=1, keepdims=True) > 1, 1 - u, u)
    a, b, c = (verts[f[:, i]].astype(np.float64) for i in range(3))
    on = a + u[:, :1] * (b - a) + u[:, 1:] * (c - a)
    return np.concatenate([box, at_verts, on]).astype(f32)


def cases():
    """{name: (points [B,N,3], verts, faces, v_count, f_count)}: the inputs of the bit comparisons of tests/test_gpu_point_mesh.py."""
    out = {}
    sv, sf = sphere_mesh()
    out["sphere"] = (sphere_queries(sv, sf, 2000, 0)[None], *pack([(sv, sf)]))
    hv, hf = huge_among_tiny()
    empty = (np.zeros((0, 3), f32), np.zeros((0, 3), np.int32))
    pts = np.stack([queries_around(sv, sf, 700, 1), queries_around(sv, sf, 700, 2), queries_around(hv, hf, 700, 3)])
    out["batch3"] = (pts, *pack([(sv, sf), empty, (hv[:3 + 3 * 200], hf[:201])]))
    out["huge"] = (queries_around(hv, hf, 1000, 4)[None], *pack([(hv, hf)]))
    dv, df = degenerate_mesh()
    dq = np.concatenate([queries_around(dv, df, 800, 5), dv[:3], (dv[:1] + dv[1:2]) * f32(0.5), dv[3:23]])
    out["degenerate"] = (dq[None], *pack([(dv, df)]))
    fv, ff = flat_mesh()
    out["flat"] = (queries_around(fv, ff, 600, 6)[None], *pack([(fv, ff)]))
    out["n1"] = (np.asarray([[[0.3, 0.2, 0.9]]], f32), *pack([(sv, sf)]))
    out["n65"] = (queries_around(sv, sf, 65, 7)[None], *pack([(sv, sf)]))
    out["f1"] = (queries_around(hv[:3], hf[:1], 300, 8)[None], *pack([(hv[:3], hf[:1])]))
    return out
