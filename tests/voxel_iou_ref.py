"""numpy restatement of sc_voxel_frame, sc_voxel_solid and sc_voxel_iou (include/shapeclipper_hip.h states the rule, csrc/voxel_solid.hip
runs it): the frame of a pair of clouds in un-fused fp32, the voxel shell, the closing by the 3x3x3 cube, the exterior by Jacobi sweeps on
the packed words (bit z of word [x, y] is voxel (x, y, z)) and the popcounts.  scipy_solid is the same solid from scipy.ndimage, which
the host test compares it with.  Input generators of the tests are at the end."""
import collections

import numpy as np

F = np.float32
U = np.uint64
MIN_RES, MAX_RES, MAX_CLOSE = 8, 64, 2
QNAN = np.array([0x7fc00000], np.uint32).view(np.float32)[0]

Solid = collections.namedtuple("Solid", ["bits", "shell_voxels", "solid_voxels", "sweeps"])


# ---- the frame ---------------------------------------------------------------------------------------------------------------------------
def frame_one(a, b, res, close):
    """a [N,3], b [M,3] fp32 -> (origin [3], pitch) fp32."""
    m = close + 1
    both = np.concatenate([np.asarray(a, F), np.asarray(b, F)])
    if not np.isfinite(both).all():
        return np.full(3, QNAN, F), F(QNAN)
    lo, hi = both.min(axis=0), both.max(axis=0)
    with np.errstate(over="ignore", invalid="ignore"):
        ext = hi - lo
        side = max(max(ext[0], ext[1]), ext[2])
        pitch = F(1.0) if side == 0 else F(side / F(res - 2 * m))
        centre = (lo + hi) * F(0.5)
        origin = centre - F(F(res) * F(0.5)) * pitch
    return origin.astype(F), F(pitch)


def voxel_frame(a, b, res, close):
    """a [B,N,3], b [B,M,3] -> (origin [B,3], pitch [B]) fp32."""
    out = [frame_one(x, y, res, close) for x, y in zip(a, b)]
    return np.stack([o for o, _ in out]).astype(F), np.array([p for _, p in out], F)


# ---- packed volumes ------------------------------------------------------------------------------------------------------------------------
def mask_of(res):
    return U(0xFFFFFFFFFFFFFFFF) if res == 64 else U((1 << res) - 1)


def pack(vol):
    """bool [R,R,R] -> uint64 [R,R]."""
    R = vol.shape[0]
    w = np.zeros((R, R), U)
    for z in range(R):
        w |= vol[:, :, z].astype(U) << U(z)
    return w


def unpack(words):
    """uint64 [R,R] -> bool [R,R,R]."""
    R = words.shape[0]
    return np.stack([((words >> U(z)) & U(1)).astype(bool) for z in range(R)], axis=-1)


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def _shift(w, axis, step, fill=0):
    """w moved by `step` along `axis`: out[i] = w[i - step], `fill` where that is outside."""
    out = np.full_like(w, fill)
    src = [slice(None)] * 2
    dst = [slice(None)] * 2
    src[axis] = slice(0, -1) if step == 1 else slice(1, None)
    dst[axis] = slice(1, None) if step == 1 else slice(0, -1)
    out[tuple(dst)] = w[tuple(src)]
    return out


def dilate(w, res):
    w = (w | (w << U(1)) | (w >> U(1))) & mask_of(res)
    w = w | _shift(w, 1, 1) | _shift(w, 1, -1)
    return w | _shift(w, 0, 1) | _shift(w, 0, -1)


def erode(w, res):
    """The outside of the grid counts as empty: bits past R - 1 are clear in w, so the shifts bring zeros in."""
    w = w & (w << U(1)) & (w >> U(1))
    w = w & _shift(w, 1, 1) & _shift(w, 1, -1)
    return w & _shift(w, 0, 1) & _shift(w, 0, -1)


def smear(v, free):
    """The fixed point of v |= ((v << 1) | (v >> 1)) & free, by the doubling fill the kernel uses."""
    up, down, pu, pd = v.copy(), v.copy(), free.copy(), free.copy()
    for s in (1, 2, 4, 8, 16, 32):
        up |= pu & (up << U(s))
        pu &= pu << U(s)
        down |= pd & (down >> U(s))
        pd &= pd >> U(s)
    return up | down


def exterior(D, res):
    """(E, sweeps): the Jacobi sweeps of the header from the border voxels not in D."""
    free = ~D & mask_of(res)
    border = np.zeros((res, res), bool)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
    E = np.where(border, free, free & (U(1) | (U(1) << U(res - 1))))
    sweeps = 0
    while True:
        v = (E | _shift(E, 0, 1) | _shift(E, 0, -1) | _shift(E, 1, 1) | _shift(E, 1, -1)) & free
        v = smear(v, free)
        sweeps += 1
        if np.array_equal(v, E):
            return E, sweeps
        E = v


# ---- the solid -----------------------------------------------------------------------------------------------------------------------------
def shell_indices(points, origin, pitch, res, close):
    """[n,3] int64 voxel indices of the points that set a voxel (finite points in a finite frame with pitch > 0)."""
    m = close + 1
    p = np.asarray(points, F)
    origin, pitch = np.asarray(origin, F), F(pitch)
    if not (np.isfinite(origin).all() and np.isfinite(pitch) and pitch > 0):
        return np.zeros((0, 3), np.int64)
    p = p[np.isfinite(p).all(axis=1)]
    with np.errstate(over="ignore", invalid="ignore"):
        q = (p - origin) / pitch
    assert q.dtype == F
    return np.clip(np.floor(q), F(m), F(res - 1 - m)).astype(np.int64)


def shell_volume(points, origin, pitch, res, close):
    i = shell_indices(points, origin, pitch, res, close)
    vol = np.zeros((res, res, res), bool)
    vol[i[:, 0], i[:, 1], i[:, 2]] = True
    return vol


def solid_one(points, origin, pitch, res, close):
    """points [N,3] -> Solid(bits uint64 [R,R], shell_voxels, solid_voxels, sweeps)."""
    assert MIN_RES <= res <= MAX_RES and 0 <= close <= MAX_CLOSE
    w = pack(shell_volume(points, origin, pitch, res, close))
    n_shell = popcount(w)
    for _ in range(close):
        w = dilate(w, res)
    E, sweeps = exterior(w, res)
    w = ~E & mask_of(res)
    for _ in range(close):
        w = erode(w, res)
    return Solid(w, n_shell, popcount(w), sweeps)


def voxel_solid(points, origin, pitch, res, close):
    """points [B,N,3], origin [B,3], pitch [B] -> Solid(bits int64 [B,R,R], shell_voxels, solid_voxels, sweeps int32 [B]): the dtypes of
    ops.voxel_solid."""
    out = [solid_one(p, o, t, res, close) for p, o, t in zip(points, origin, pitch)]
    return Solid(np.stack([s.bits for s in out]).view(np.int64), *(np.array([s[k] for s in out], np.int32) for k in (1, 2, 3)))


def voxel_iou(bits_a, bits_b):
    """int64 [B,...] x 2 -> (inter [B], union [B]) int32."""
    a, b = np.ascontiguousarray(bits_a).view(U), np.ascontiguousarray(bits_b).view(U)
    return (np.array([popcount(x & y) for x, y in zip(a, b)], np.int32), np.array([popcount(x | y) for x, y in zip(a, b)], np.int32))


def iou_value(inter, union):
    """float64 inter / union, 1 for an empty union."""
    inter, union = np.asarray(inter, np.float64), np.asarray(union, np.float64)
    return np.where(union > 0, inter / np.maximum(union, 1.0), 1.0)


def pair_iou(a, b, res, close):
    """a [N,3], b [M,3] -> (iou, inter, union, Solid of a, Solid of b) in the pair's frame; iou NaN for a frame that is not finite."""
    origin, pitch = frame_one(a, b, res, close)
    sa, sb = solid_one(a, origin, pitch, res, close), solid_one(b, origin, pitch, res, close)
    inter, union = popcount(sa.bits & sb.bits), popcount(sa.bits | sb.bits)
    ok = np.isfinite(origin).all() and np.isfinite(pitch)
    return (float(iou_value(inter, union)) if ok else float("nan")), inter, union, sa, sb


def scipy_solid(shell, close):
    """bool [R,R,R] -> binary_erosion(binary_fill_holes(binary_dilation(shell, cube, close)), cube, close); iterations = 0 would mean
    'until nothing changes' to scipy, so close = 0 skips the two calls."""
    from scipy import ndimage
    cube = np.ones((3, 3, 3), bool)
    D = ndimage.binary_dilation(shell, cube, iterations=close) if close else shell
    filled = ndimage.binary_fill_holes(D)
    return ndimage.binary_erosion(filled, cube, iterations=close) if close else filled


# ---- inputs of the tests -------------------------------------------------------------------------------------------------------------------
def sphere(n, seed=0, radius=0.5):
    d = np.random.RandomState(seed).randn(n, 3)
    return (radius * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)


def torus(n, seed=0, major=0.35, minor=0.12):
    u, v = np.random.RandomState(seed).uniform(0, 2 * np.pi, (2, n))
    r = major + minor * np.cos(v)
    return np.stack([r * np.cos(u), r * np.sin(u), minor * np.sin(v)], axis=1).astype(F)


def box_surface(n, half=(0.5, 0.3, 0.2), centre=(0, 0, 0), seed=0):
    """n points uniform on the surface of the axis-aligned box: a face by its area, a point on it uniformly."""
    rng = np.random.RandomState(seed)
    h = np.asarray(half, np.float64)
    area = np.array([h[1] * h[2], h[0] * h[2], h[0] * h[1]])
    axis = rng.choice(3, n, p=area / area.sum())
    p = rng.uniform(-1, 1, (n, 3)) * h
    p[np.arange(n), axis] = rng.choice([-1.0, 1.0], n) * h[axis]
    return (p + np.asarray(centre)).astype(F)


def chair(n, seed=0):
    """Six thin boxes: seat, back and four legs."""
    parts = [((0.25, 0.25, 0.03), (0, 0, 0)), ((0.25, 0.03, 0.25), (0, 0.22, 0.28)),
             ((0.03, 0.03, 0.2), (-0.2, -0.2, -0.23)), ((0.03, 0.03, 0.2), (0.2, -0.2, -0.23)),
             ((0.03, 0.03, 0.2), (-0.2, 0.2, -0.23)), ((0.03, 0.03, 0.2), (0.2, 0.2, -0.23))]
    k = n // len(parts)
    return np.concatenate([box_surface(k + (n - k * len(parts) if i == 0 else 0), half, centre, seed=seed + i)
                           for i, (half, centre) in enumerate(parts)])


def perturbed(p, seed=1, scale=1.05, shift=0.03):
    """A copy of the cloud, scaled, moved and in another order: the other cloud of a pair."""
    rng = np.random.RandomState(seed)
    return (p[rng.permutation(len(p))].astype(np.float64) * scale + shift * rng.uniform(-1, 1, 3)).astype(F)


SHAPES = {"sphere": sphere, "torus": torus, "box": box_surface, "chair": chair}


def shape_pair(name, n=20000, seed=0):
    a = SHAPES[name](n, seed=seed)
    return a, perturbed(a, seed=seed + 1)


def serpentine(res):
    """(points [N,3], origin [3], pitch): voxel centres in the frame origin 0, pitch 1 of a closed box over indices 1 .. res - 2 (close
    = 0) with one hole in its x = 1 wall and, inside, walls across x at every second y, each open at one alternating end and reaching
    from lid to lid -- the exterior enters by the hole and has to walk every corridor, one voxel of x or y per sweep.  In the end it
    has reached all of the inside: the solid is the shell."""
    lo, hi = 1, res - 2
    vol = np.zeros((res, res, res), bool)
    vol[lo:hi + 1, lo:hi + 1, [lo, hi]] = True
    vol[[lo, hi], lo:hi + 1, lo:hi + 1] = True
    vol[lo:hi + 1, [lo, hi], lo:hi + 1] = True
    vol[lo, lo + 1, res // 2] = False                           # the hole, into the first corridor y = lo + 1
    for k, y in enumerate(range(lo + 2, hi - 1, 2)):
        vol[lo + 1:hi, y, lo:hi + 1] = True
        vol[hi - 1 if k % 2 == 0 else lo + 1, y, lo + 1:hi] = False
    idx = np.argwhere(vol)
    return (idx + 0.5).astype(F), np.zeros(3, F), F(1.0)
