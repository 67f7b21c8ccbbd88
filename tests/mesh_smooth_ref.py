"""numpy restatement of sc_mesh_smooth (include/shapeclipper_hip.h): the rules of ops.mesh_smooth for ONE image -- the distinct edges of
every face and their counts, the neighbour rows in ascending order, the fixed rim, the float64 Jacobi half-steps with one rounding per
operation, the fp32 output and the measures with the header's chunked sums.  numpy's elementwise float64 operations round once each and
never fuse, which is what the kernel is built to do.  Also the shapes that the host and GPU tests share."""
import numpy as np

CHUNK = 256         # SC_MESH_SMOOTH_CHUNK
MAX_ITERS = 1000    # SC_MESH_SMOOTH_MAX_ITERS
LAM = 0.5
MU = 1.0 / (0.1 - 1.0 / 0.5)        # Taubin's pass-band 0.1 at lam 0.5: -0.5263157894736842
INTS = ("free", "fixed_boundary", "isolated", "degree_max")
MEASURES = ("rough_before", "rough_after", "disp_mean", "disp_max")


def edge_counts(faces, V):
    """{(lo, hi): faces that have the edge}: every face gives each of its distinct undirected edges once.  ValueError("bad_index") for a
    face index outside [0, V)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(faces) and (faces.min() < 0 or faces.max() >= V):
        raise ValueError("bad_index")
    count = {}
    for a, b, c in faces.tolist():
        for e in {(min(p, q), max(p, q)) for p, q in ((a, b), (b, c), (c, a)) if p != q}:
            count[e] = count.get(e, 0) + 1
    return count


def neighbours(faces, V):
    """-> (rows, fixed): rows[i] the ascending list of N(i), fixed [V] bool the vertices on an edge of count 1."""
    rows, fixed = [set() for _ in range(V)], np.zeros(V, bool)
    for (lo, hi), n in edge_counts(faces, V).items():
        rows[lo].add(hi)
        rows[hi].add(lo)
        if n == 1:
            fixed[lo] = fixed[hi] = True
    return [sorted(r) for r in rows], fixed


def _means(x, table, degree):
    """m [V,3]: per row 0.0 plus x_j in ascending j, one addition at a time, over the float64 degree (rows without a neighbour: nan)."""
    s = np.zeros_like(x)
    for k in range(table.shape[1]):
        has = degree > k
        s[has] = s[has] + x[table[has, k]]
    with np.errstate(all="ignore"):
        return s / degree.astype(np.float64)[:, None]


def _norm(d):
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def _chunked(terms, fold):
    """0.0 folded with the chunk partials in ascending chunk number, a partial being 0.0 folded with its terms in ascending order."""
    total = np.float64(0.0)
    for first in range(0, len(terms), CHUNK):
        part = np.float64(0.0)
        for t in terms[first:first + CHUNK]:
            part = fold(part, t)
        total = fold(total, part)
    return total


def mesh_smooth(verts, faces, iters, lam=LAM, mu=MU):
    """verts [V,3] float32, faces [F,3] integers of one image -> dict of verts [V,3] float32, fixed_mask [V] bool (the vertices on an
    edge of count 1), the four INTS (ints) and the four MEASURES (np.float64).  ValueError("bad_vertex") / ("bad_index") where
    the kernel sets its flags."""
    assert isinstance(iters, int) and 0 <= iters <= MAX_ITERS and 0.0 < lam <= 1.0 and -1.0 <= mu <= 0.0
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    V = len(verts)
    if not np.isfinite(verts).all():
        raise ValueError("bad_vertex")
    rows, fixed = neighbours(faces, V)
    degree = np.array([len(r) for r in rows], np.int64).reshape(V)
    table = np.zeros((V, int(degree.max()) if V else 0), np.int64)
    for i, r in enumerate(rows):
        table[i, :len(r)] = r
    free = (degree > 0) & ~fixed
    start = verts.astype(np.float64)
    x = start.copy()
    for _ in range(iters):
        for factor in (lam, mu) if mu != 0.0 else (lam,):
            m = _means(x, table, degree)
            d = m[free] - x[free]
            t = np.float64(factor) * d
            new = x.copy()
            new[free] = x[free] + t
            x = new
    out = verts.copy()
    out[free] = x[free].astype(np.float32)
    n_free = int(free.sum())

    def rough(state):
        return np.where(free, _norm(np.where(free[:, None], _means(state, table, degree) - state, 0.0)), 0.0)

    moved = np.where(free, _norm(x - start), 0.0)
    add, top = (lambda acc, t: acc + t), (lambda acc, t: t if t > acc else acc)
    mean = lambda terms: _chunked(terms, add) / np.float64(n_free) if n_free else np.float64(0.0)
    return dict(verts=out, fixed_mask=fixed, free=n_free, fixed_boundary=int(fixed.sum()), isolated=int((degree == 0).sum()),
                degree_max=int(degree.max()) if V else 0, rough_before=mean(rough(start)), rough_after=mean(rough(x)), disp_mean=mean(moved),
                disp_max=_chunked(moved, top) if n_free else np.float64(0.0))


# ---- the hand-made shapes of the tests ---------------------------------------------------------------------------------------------------
OCTA_V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
OCTA_F = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)

# a hexagon fan: the rim, counter-clockwise, then the hub above its centre
HEX_V = np.array([[2, 0, 0], [1, 2, 0], [-1, 2, 0], [-2, 0, 0], [-1, -2, 0], [1, -2, 0], [0, 0, 1]], np.float32)
HEX_F = np.array([[6, k, (k + 1) % 6] for k in range(6)], np.int32)


def double_cone(spokes=300):
    """A closed double cone: `spokes` rim vertices on the unit circle (slightly uneven in height), an apex above (vertex `spokes`) and one
    below (`spokes` + 1).  Both apexes have `spokes` neighbours, every rim vertex four."""
    a = 2.0 * np.pi * np.arange(spokes) / spokes
    rim = np.stack([np.cos(a), np.sin(a), 0.05 * np.sin(7.0 * a)], axis=1)
    verts = np.concatenate([rim, [[0.0, 0.0, 1.0], [0.0, 0.0, -1.3]]]).astype(np.float32)
    k = np.arange(spokes)
    n = (k + 1) % spokes
    top = np.stack([np.full(spokes, spokes), k, n], axis=1)
    bottom = np.stack([np.full(spokes, spokes + 1), n, k], axis=1)
    return verts, np.concatenate([top, bottom]).astype(np.int32)


def cut_sphere_level():
    """A 17^3 level grid of a sphere whose centre lies near the grid's x = 0 face: marching cubes leaves the surface open there."""
    g = np.arange(17, dtype=np.float64)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    return (np.sqrt((x - 1.3) ** 2 + (y - 7.9) ** 2 + (z - 8.2) ** 2) - 5.3).astype(np.float32)


_MESH = {}


def shape(name):
    """The indexed marching-cubes mesh (grid-index units) of mesh_simplify_ref's 17^3 shapes, or of "cut_sphere"; built once."""
    import mesh_simplify_ref
    if name != "cut_sphere":
        return mesh_simplify_ref.mc_mesh(name)
    if name not in _MESH:
        mesh_simplify_ref.mc_mesh("sphere")                 # puts the repository root on sys.path
        from oracle import isosurface_ref
        _MESH[name] = mesh_simplify_ref.indexed(isosurface_ref.marching_cubes(cut_sphere_level()))
    return _MESH[name]
