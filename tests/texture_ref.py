"""numpy restatement of the per-triangle texture atlas (include/shapeclipper_hip.h: layout, sc_texture_queries, sc_texture_pack,
sc_texture_sample) and the meshes its tests run on.  Not a test module.

Everything that the kernels compute in fp32 is computed here in np.float32, one operation per line where the order matters, so the
GPU tests compare bit for bit.  One image at a time; the callers loop over the batch."""
import numpy as np

F32 = np.float32
T_RANGE = range(4, 33)
A_MIN, A_MAX = 64, 8192


def layout(f_max, T):
    """(A, n, rows): the smallest power of two A in 64..8192 with n = A // T and n n >= ceil(f_max / 2); rows = T ceil(cells / n)."""
    cells = (f_max + 1) // 2
    A = A_MIN
    while (A // T) ** 2 < cells:
        A *= 2
        if A > A_MAX:
            raise ValueError("eval.texture_texels = %d: %d faces do not fit an atlas of %d" % (T, f_max, A_MAX))
    n = A // T
    return A, n, T * ((cells + n - 1) // n)


def corners(T, h):
    """Cell-local texel indices [3,2] (x, y) of the chart corners p0, p1, p2 of half h."""
    if h == 0:
        return np.array([[0, 0], [T - 3, 0], [0, T - 3]], np.int64)
    return np.array([[T - 1, T - 1], [2, T - 1], [T - 1, 2]], np.int64)


def cell_origin(f, n, T):
    """(X0, Y0) of the cell of face(s) f."""
    c = np.asarray(f, np.int64) >> 1
    return T * (c % n), T * (c // n)


def texel_faces(A, T, F, rows=None):
    """(face [rows, A] int32 with -1 where unused, i, j, h [rows, A]): the face every texel of rows [0, rows) belongs to."""
    n = A // T
    rows = A if rows is None else rows
    y, x = np.meshgrid(np.arange(rows, dtype=np.int64), np.arange(A, dtype=np.int64), indexing="ij")
    cx, cy = x // T, y // T
    i, j = x - cx * T, y - cy * T
    h = (i + j > T - 1).astype(np.int64)
    f = 2 * (cy * n + cx) + h
    used = (cx < n) & (cy < n) & (f < F)
    return np.where(used, f, -1).astype(np.int32), i, j, h


def texel_barycentrics(i, j, h, T):
    """fp32 (b0, b1, b2) of texels (i, j) of half h: the header's expressions."""
    d = F32(T - 3)
    b1 = np.where(h == 1, T - 1 - i, i).astype(F32) / d
    b2 = np.where(h == 1, T - 1 - j, j).astype(F32) / d
    b0 = (F32(1) - b1) - b2
    return b0, b1, b2


def face_uv(F, A, T):
    """OBJ texture coordinates [F,3,2] float64 (exact, and exactly representable in fp32) of the corners of faces 0..F-1."""
    n = A // T
    f = np.arange(F, dtype=np.int64)
    X0, Y0 = cell_origin(f, n, T)
    p = np.stack([corners(T, 0), corners(T, 1)])[f & 1]                # [F,3,2]
    u = (X0[:, None] + p[..., 0] + 0.5) / A
    v = 1.0 - (Y0[:, None] + p[..., 1] + 0.5) / A
    return np.stack([u, v], -1)


def scale_of(lo, hi, S):
    return F32((float(hi) - float(lo)) / float(S - 1))


def queries(verts, faces, A, T, lo, hi, S, rows):
    """One image: verts [V,3] fp32 (grid-index units), faces [F,3] int -> (query [rows A, 3] fp32, face_of_texel [rows A] int32)."""
    verts, faces = np.asarray(verts, F32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(faces)
    face, i, j, h = texel_faces(A, T, F, rows)
    lo32, scale = F32(lo), scale_of(lo, hi, S)
    out = np.full((rows, A, 3), lo32, F32)
    if F > 0:
        used = face >= 0
        # unused texels: texel (0, 0) of the image, i.e. face 0 at i = j = 0 of the lower half
        fi = np.where(used, face, 0).astype(np.int64)
        ii, jj, hh = np.where(used, i, 0), np.where(used, j, 0), np.where(used, h, 0)
        b0, b1, b2 = texel_barycentrics(ii, jj, hh, T)
        v0, v1, v2 = (verts[faces[fi, k]] for k in range(3))            # [rows, A, 3]
        t0 = b0[..., None] * v0
        t1 = b1[..., None] * v1
        t2 = b2[..., None] * v2
        p = (t0 + t1) + t2
        out = lo32 + p * scale
    return out.reshape(-1, 3).astype(F32), face.reshape(-1)


def unit_byte(v):
    v = np.asarray(v, F32)
    c = np.where(v < 0, F32(0), np.where(v > 1, F32(1), v)).astype(F32)
    with np.errstate(invalid="ignore"):
        b = (c * F32(255)).astype(F32)
    return np.where(np.isnan(v), 0, np.nan_to_num(b)).astype(np.uint8)


def pack(rgb, normal, face_of_texel, A, rows):
    """One image: rgb, normal [rows A, 3] fp32, face_of_texel [rows A] -> (atlas, normal_atlas) uint8 [A, A, 3]."""
    atlas = np.full((A, A, 3), 127, np.uint8)
    atlas_n = np.full((A, A, 3), 127, np.uint8)
    used = (np.asarray(face_of_texel).reshape(rows, A) >= 0)[..., None]
    c = unit_byte(np.asarray(rgb, F32).reshape(rows, A, 3))
    m = unit_byte((np.asarray(normal, F32).reshape(rows, A, 3) + F32(1)) * F32(0.5))
    atlas[:rows] = np.where(used, c, 127)
    atlas_n[:rows] = np.where(used, m, 127)
    return atlas, atlas_n


def footprint(uv, A):
    """uv [N,2] fp32 -> (xa, xb, ya, yb int64 [N], fx, fy fp32 [N]): the clamped columns / rows and weights of the bilinear look-up."""
    uv = np.asarray(uv, F32)
    fA = F32(A)
    x = uv[:, 0] * fA - F32(0.5)
    y = (F32(1) - uv[:, 1]) * fA - F32(0.5)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0).astype(F32), (y - y0).astype(F32)

    def pair(f0):
        k = np.fmax(np.fmin(f0, fA), F32(-1)).astype(np.int64)
        return np.clip(k, 0, A - 1), np.clip(k + 1, 0, A - 1)
    xa, xb = pair(x0)
    ya, yb = pair(y0)
    return xa, xb, ya, yb, fx, fy


def sample(atlas, uv):
    """One image: atlas [A, A, C] (fp32 or uint8), uv [N,2] fp32 -> [N, C] fp32, the header's expression in its order."""
    A = atlas.shape[0]
    t = np.asarray(atlas).astype(F32)
    xa, xb, ya, yb, fx, fy = footprint(uv, A)
    fx, fy = fx[:, None], fy[:, None]
    gx, gy = F32(1) - fx, F32(1) - fy
    top = gx * t[ya, xa] + fx * t[ya, xb]
    bot = gx * t[yb, xa] + fx * t[yb, xb]
    return (top * gy + bot * fy).astype(F32)


# ---- the level grids of the GPU tests: analytic spheres, as the other meshing tests use ------------------------------------------------
def sphere_level(S, radius, centre=(0.0, 0.0, 0.0), lo=-0.5, hi=0.5):
    """|x - centre| - radius on the S^3 grid over [lo, hi]^3, fp32."""
    g = np.linspace(lo, hi, S)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    c = centre
    return (np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - radius).astype(F32)


def two_sphere_level(S, lo=-0.5, hi=0.5):
    """The union of two spheres: enough faces at S = 32 for an atlas above 64 at every tested T."""
    return np.minimum(sphere_level(S, 0.27, (-0.2, -0.1, 0.0), lo, hi), sphere_level(S, 0.33, (0.15, 0.1, 0.05), lo, hi))


def empty_level(S):
    return np.ones((S, S, S), F32)
