"""numpy restatement of csrc/point_normals.hip as include/shapeclipper_hip.h states it: the k-NN keys in fp32 (bit for bit), the PCA
normals in float64 (op for op: mean and covariance in rank order, 8 cyclic two-sided Jacobi sweeps, the sign rule, one rounding to
fp32) and the normal consistency in float64.  Test clouds for tests/test_gpu_point_normals.py and tests/test_point_normals_host.py."""
import numpy as np

SWEEPS = 8


# ---- k nearest neighbours ----------------------------------------------------------------------------------------------------------
def knn_keys(points, i):
    """uint64 keys (bits(d) << 32) | j of query i against all points j of one cloud [N,3] fp32; d = (dx dx + dy dy) + dz dz in fp32."""
    p = np.asarray(points, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = p[:, 0] - p[i, 0], p[:, 1] - p[i, 1], p[:, 2] - p[i, 2]
        d = ((dx * dx + dy * dy) + dz * dz).astype(np.float32)
    return (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(p), dtype=np.uint64)


def knn(points, k):
    """points [N,3] fp32 -> (idx [N,k] int32, dist [N,k] fp32): the k smallest keys of every row of the all-pairs table, ascending."""
    p = np.asarray(points, np.float32)
    N = len(p)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = p[None, :, 0] - p[:, None, 0]
        dy = p[None, :, 1] - p[:, None, 1]
        dz = p[None, :, 2] - p[:, None, 2]
        d = ((dx * dx + dy * dy) + dz * dz).astype(np.float32)
    keys = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(N, dtype=np.uint64)[None]
    keys = np.sort(keys, axis=1)[:, :k]
    idx = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    dist = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return idx, dist


# ---- PCA normals -------------------------------------------------------------------------------------------------------------------
def covariance(points, idx):
    """points [N,3], idx [N,k] (inside 0..N-1) -> (m [N,3], C dict (a, b) -> [N]) float64, both summed in rank order and divided by k."""
    q = np.asarray(points, np.float32).astype(np.float64)[idx]           # [N, k, 3]
    k = idx.shape[1]
    m = np.zeros((len(idx), 3))
    for r in range(k):
        m = m + q[:, r]
    m = m / float(k)
    C = {(a, b): np.zeros(len(idx)) for a in range(3) for b in range(a, 3)}
    for r in range(k):
        d = q[:, r] - m
        for (a, b) in C:
            C[(a, b)] = C[(a, b)] + d[:, a] * d[:, b]
    for key in C:
        C[key] = C[key] / float(k)
    return m, C


def jacobi(C, sweeps=SWEEPS):
    """C dict (a, b) -> [N] float64 (a <= b) -> (diag [N,3], V [N,3,3], V[:, :, c] the vector of diag[:, c]): `sweeps` cyclic sweeps over
    (0,1), (0,2), (1,2) with the header's rotation."""
    A = {key: np.array(v, np.float64) for key, v in C.items()}
    N = len(A[(0, 0)])
    V = np.tile(np.eye(3), (N, 1, 1))
    sym = lambda a, b: (a, b) if a <= b else (b, a)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
                app, aqq, apq = A[(p, p)], A[(q, q)], A[(p, q)]
                arp, arq = A[sym(r, p)], A[sym(r, q)]
                on = apq != 0.0
                safe = np.where(on, apq, 1.0)
                theta = (aqq - app) / (2.0 * safe)
                big = np.abs(theta) > 1.0e150
                th = np.where(big, 1.0, theta)
                t = np.where(big, 0.5 / np.where(theta == 0.0, 1.0, theta), np.where(th < 0.0, -1.0, 1.0) / (np.abs(th) + np.sqrt(th * th + 1.0)))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                h = t * apq
                A[(p, p)] = np.where(on, app - h, app)
                A[(q, q)] = np.where(on, aqq + h, aqq)
                A[(p, q)] = np.where(on, 0.0, apq)
                A[sym(r, p)] = np.where(on, c * arp - s * arq, arp)
                A[sym(r, q)] = np.where(on, s * arp + c * arq, arq)
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p] = np.where(on[:, None], c[:, None] * vp - s[:, None] * vq, vp)
                V[:, :, q] = np.where(on[:, None], s[:, None] * vp + c[:, None] * vq, vq)
    return np.stack([A[(0, 0)], A[(1, 1)], A[(2, 2)]], axis=1), V


def normals(points, idx):
    """points [N,3] fp32, idx [N,k] -> (normals [N,3] fp32, variation [N] fp32, eig [N,3] float64 ascending), the header's definition;
    an index outside 0..N-1 counts as a NaN point."""
    p = np.asarray(points, np.float32)
    idx = np.asarray(idx)
    inside = (idx >= 0) & (idx < len(p))
    pad = np.concatenate([p, np.full((1, 3), np.nan, np.float32)])
    m, C = covariance(pad, np.where(inside, idx, len(p)))
    diag, V = jacobi(C)
    order = np.argsort(diag, axis=1, kind="stable")
    lam = np.take_along_axis(diag, order, axis=1)
    vec = np.take_along_axis(V, order[:, None, :1].repeat(3, axis=1), axis=2)[:, :, 0]
    big = np.argmax(np.abs(vec), axis=1)                                 # the first one on a tie
    sign = np.where(np.take_along_axis(vec, big[:, None], axis=1)[:, 0] < 0.0, -1.0, 1.0)
    with np.errstate(all="ignore"):
        finite = np.isfinite(m).all(axis=1) & np.all([np.isfinite(v) for v in C.values()], axis=0) & np.isfinite(lam).all(axis=1)
        ok = finite & ~(lam[:, 1] <= 1.0e-12 * lam[:, 2])
        var = lam[:, 0] / ((lam[:, 0] + lam[:, 1]) + lam[:, 2])
    n = np.where(ok[:, None], sign[:, None] * vec, 0.0).astype(np.float32)
    return n, np.where(ok, var, 0.0).astype(np.float32), lam


def jacobi_against_eigh(points, idx):
    """Worst |difference| over all points between the 8-sweep Jacobi normal and numpy.linalg.eigh's (up to sign), and between the
    eigenvalues, for well-separated points ((l1 - l0) / l2 >= 1e-3)."""
    _, C = covariance(points, idx)
    diag, V = jacobi(C)
    M = np.zeros((len(idx), 3, 3))
    for (a, b), v in C.items():
        M[:, a, b] = v
        M[:, b, a] = v
    w, U = np.linalg.eigh(M)
    order = np.argsort(diag, axis=1, kind="stable")
    lam = np.take_along_axis(diag, order, axis=1)
    vec = np.take_along_axis(V, order[:, None, :1].repeat(3, axis=1), axis=2)[:, :, 0]
    keep = (lam[:, 1] - lam[:, 0]) / lam[:, 2] >= 1e-3
    u = U[:, :, 0]
    dv = np.minimum(np.abs(vec - u).max(axis=1), np.abs(vec + u).max(axis=1))
    return float(dv[keep].max()), float(np.abs(lam - w)[keep].max()), int(keep.sum())


# ---- normal consistency ------------------------------------------------------------------------------------------------------------
def normal_consistency(n1, n2, idx1, idx2):
    """One image: (acc, comp) float64, mean |n1[i] . n2[idx1[i]]| and mean |n2[j] . n1[idx2[j]]|; NaN for an index outside its cloud."""
    a, b = np.asarray(n1, np.float32).astype(np.float64), np.asarray(n2, np.float32).astype(np.float64)

    def half(own, oth, idx):
        idx = np.asarray(idx)
        inside = (idx >= 0) & (idx < len(oth))
        o = oth[np.where(inside, idx, 0)]
        dots = np.abs((own[:, 0] * o[:, 0] + own[:, 1] * o[:, 1]) + own[:, 2] * o[:, 2])
        return float(np.where(inside, dots, np.nan).sum() / len(own))

    return half(a, b, idx1), half(b, a, idx2)


# ---- clouds ------------------------------------------------------------------------------------------------------------------------
def volume(seed, n, images=None):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.5, 0.5, (n, 3) if images is None else (images, n, 3)).astype(np.float32)


def sphere(seed, n, radius=0.5):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    return (radius * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def cube_surface(seed, n):
    """n points uniform on the surface of the unit cube [-0.5, 0.5]^3 -> (points [n,3] fp32, axis [n] of the face's normal)."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.5, 0.5, (n, 3))
    axis = rng.integers(0, 3, n)
    p[np.arange(n), axis] = np.where(rng.integers(0, 2, n) == 0, -0.5, 0.5)
    return p.astype(np.float32), axis


def with_duplicates(seed, n, copies=50):
    p = volume(seed, n)
    p[n - copies:] = p[7]
    return p


def with_outlier(seed, n):
    p = volume(seed, n)
    p[n // 2] = np.float32([40.0, -25.0, 60.0])
    return p
