"""numpy float64 restatement of the evaluation's similarity ICP (ops.icp_fit / icp_apply / icp_align; include/shapeclipper_hip.h states
the definition) and the inputs its tests share.  No GPU, no torch.

The restatement follows the header's definition with numpy's own summation order and LAPACK's SVD, so a fit agrees with the kernels
to rounding (about N 2^-53 on well-conditioned clouds), not bit for bit; `apply` IS bit for bit: numpy rounds every float64 operation
once and the kernel is built without contraction."""
import numpy as np

SEEDS = (0, 1, 2, 3)
# (angle in degrees, |t0|, s0, scale fitted)
CASES = ((10.0, 0.05, 1.1, True), (15.0, 0.03, 0.9, True), (10.0, 0.05, 1.0, False), (20.0, 0.08, 1.15, True))
N_POINTS = 1024
BOXES = (((-.3, -.05, -.3), (.3, .05, .3)),        # seat, n / 2 points
         ((-.3, .05, .2), (.3, .55, .3)),          # back, n / 4
         ((.15, -.5, -.3), (.3, -.05, -.15)))      # leg, the rest


def chair(n, rng):
    """[n,3] fp32: points uniform on the faces of the three boxes -- a uniform point in the box, then a random axis snapped to a random
    side."""
    counts = (n // 2, n // 4, n - n // 2 - n // 4)
    parts = []
    for (lo, hi), k in zip(BOXES, counts):
        lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        p = rng.uniform(lo, hi, size=(k, 3))
        axis = rng.integers(0, 3, size=k)
        side = rng.integers(0, 2, size=k)
        p[np.arange(k), axis] = np.where(side == 0, lo[axis], hi[axis])
        parts.append(p)
    return np.concatenate(parts).astype(np.float32)


def rotation(axis, angle_deg):
    """Rodrigues: the float64 rotation by angle_deg about axis."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(angle_deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def similar_pair(src, rng, angle_deg, t_norm, s0):
    """-> (dst [n,3] fp32 = fp32(s0 R0 src + t0) in float64, then permuted; R0, t0, inverse permutation): dst[inv[i]] is src[i]'s image.
    The axis of R0 and the direction of t0 come from rng."""
    R0 = rotation(rng.normal(size=3), angle_deg)
    t0 = rng.normal(size=3)
    t0 = t0 / np.linalg.norm(t0) * t_norm
    moved = (s0 * (src.astype(np.float64) @ R0.T) + t0).astype(np.float32)
    perm = rng.permutation(len(src))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(src))
    return moved[perm], R0, t0, inv


def case(seed, k, n=N_POINTS):
    """Case k of CASES for seed: dict(src, dst, R0, t0, s0, scale, inv)."""
    angle, t_norm, s0, scale = CASES[k]
    rng = np.random.default_rng(seed)
    src = chair(n, rng)
    dst, R0, t0, inv = similar_pair(src, rng, angle, t_norm, s0)
    return dict(src=src, dst=dst, R0=R0, t0=t0, s0=s0, scale=scale, inv=inv.astype(np.int32))


def all_cases(n=N_POINTS):
    return [case(seed, k, n) for seed in SEEDS for k in range(len(CASES))]


def unmatched_case():
    """The case without true correspondences: a chair of 1,024 points against an independent chair of 1,500 points moved by 12 degrees
    about (1, 2, 3), scale 1.08 and t = (.03, -.02, .04)."""
    src = chair(1024, np.random.default_rng(100))
    other = chair(1500, np.random.default_rng(101))
    R0 = rotation((1.0, 2.0, 3.0), 12.0)
    dst = (1.08 * (other.astype(np.float64) @ R0.T) + np.array([.03, -.02, .04])).astype(np.float32)
    return src, dst


def nearest(a, b):
    """fp32 squared distances by differences, ((dx dx + dy dy) + dz dz), all pairs: (dist [n] fp32, idx [n] int32, first index on ties) of
    a's points in b."""
    d = None
    for c in range(3):
        diff = a[:, None, c] - b[None, :, c]
        d = diff * diff if d is None else d + diff * diff
    idx = d.argmin(axis=1)
    return d[np.arange(len(a)), idx], idx.astype(np.int32)


def search(cur, dst):
    d1, i1 = nearest(cur, dst)
    d2, i2 = nearest(dst, cur)
    return d1, d2, i1, i2


def objective(d1, d2):
    return d1.astype(np.float64).mean() + d2.astype(np.float64).mean()


IDENTITY = np.eye(4)


def fit(src, dst, idx1, idx2, scale=True, prev=(IDENTITY, 1.0)):
    """One image: src [n,3], dst [m,3] fp32, idx1 [n], idx2 [m] -> (transform [4,4] float64, s).  The header's sc_icp_fit."""
    p = [src.astype(np.float64), src[idx2].astype(np.float64)]
    q = [dst[idx1].astype(np.float64), dst.astype(np.float64)]
    mean = lambda f: (f[0].sum(axis=0) / len(f[0]) + f[1].sum(axis=0) / len(f[1])) / 2
    pm, qm = mean(p), mean(q)
    dp, dq = [x - pm for x in p], [x - qm for x in q]
    H = mean([(b[:, :, None] * a[:, None, :]) for a, b in zip(dp, dq)])
    var_p = mean([(a * a).sum(axis=1) for a in dp])
    if not (np.isfinite(pm).all() and np.isfinite(qm).all() and np.isfinite(H).all() and np.isfinite(var_p)) or not var_p > 0:
        return prev[0].copy(), prev[1]
    U, D, Vt = np.linalg.svd(H)
    if not D[1] > 1e-12 * D[0]:
        return prev[0].copy(), prev[1]
    sign = 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0 else -1.0
    R = U @ np.diag([1.0, 1.0, sign]) @ Vt
    s = (D[0] + D[1] + sign * D[2]) / var_p if scale else 1.0
    T = np.eye(4)
    T[:3, :3] = s * R
    T[:3, 3] = qm - T[:3, :3] @ pm
    if not np.isfinite(T).all():
        return prev[0].copy(), prev[1]
    return T, s


def apply(src, T):
    """fp32(((m0 x + m1 y) + m2 z) + t) per coordinate, float64 inside: sc_icp_apply bit for bit.  src [..., 3] fp32, T [4,4]."""
    x, y, z = (src[..., c].astype(np.float64) for c in range(3))
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([(((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]).astype(np.float32) for r in range(3)], axis=-1)


def align(src, dst, iters=30, scale=True):
    """One image: dict(transform, s, aligned, dist1, dist2, idx1, idx2, objective [iters+1]).  Once a search returns the indices of the
    search before it, the absolute fit returns the same transform and every later round repeats: the loop stops there and fills the
    rest of `objective` with the repeated value, which is what the full count gives."""
    T, s = np.eye(4), 1.0
    obj = np.empty(iters + 1)
    last = None
    for j in range(iters + 1):
        cur = apply(src, T)
        d1, d2, i1, i2 = search(cur, dst)
        obj[j] = objective(d1, d2)
        if last is not None and np.array_equal(i1, last[0]) and np.array_equal(i2, last[1]):
            obj[j:] = obj[j]
            break
        last = (i1, i2)
        if j < iters:
            T, s = fit(src, dst, i1, i2, scale, prev=(T, s))
    return dict(transform=T, s=s, aligned=cur, dist1=d1, dist2=d2, idx1=i1, idx2=i2, objective=obj)
