"""numpy restatement of sc_mesh_cluster_simplify (include/shapeclipper_hip.h): the rules of ops.mesh_cluster_simplify for ONE image --
cells, clusters in ascending cell id, int64 accumulators of values rounded at 2^-24, the float64 solve in the header's order, the
collapse, the parity groups and the cancellation.  numpy's elementwise float64 operations round once each and never fuse, which is what
the kernel is built to do.  Also the level grids and the indexed marching-cubes meshes the host and GPU tests share."""
import os
import sys

import numpy as np

SCALE = np.float64(2.0 ** 24)
CLAMP = np.float64(2.0 ** 12)
MAX_CELLS = 128     # SC_MESH_SIMPLIFY_MAX_CELLS


def _fix(t):
    """llrint(clamp(t, -2^12, 2^12) 2^24) as int64."""
    t = np.where(t > CLAMP, CLAMP, np.where(t < -CLAMP, -CLAMP, t))
    return np.rint(t * SCALE).astype(np.int64)


def locate(verts, origin, pitch, cells):
    """-> (q [V,3] float64, cell [V,3] int64, bad [V] bool)."""
    p = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    o = np.asarray(origin, np.float32).astype(np.float64)
    h = np.float64(np.float32(pitch))
    with np.errstate(all="ignore"):
        q = (p - o) / h
        bad = ~(np.isfinite(p) & (q >= 0.0) & (q <= np.float64(cells))).all(axis=1)
        cell = np.minimum(np.floor(np.where(bad[:, None], 0.0, q)), cells - 1).astype(np.int64)
    return q, cell, bad


def solve(acc, reg):
    """acc [K,13] int64 -> x [K,3] float64 in [-0.5, 0.5], the header's solve."""
    inv = np.float64(1.0) / SCALE
    a = acc.astype(np.float64)
    n = a[:, 0]
    c = [a[:, 1 + j] * inv / n for j in range(3)]
    a00, a01, a02, a11, a12, a22 = (a[:, 4 + t] * inv for t in range(6))
    b = [a[:, 10 + j] * inv for j in range(3)]
    lam = np.float64(reg) * ((a00 + a11) + a22)
    with np.errstate(all="ignore"):
        a00, a11, a22 = a00 + lam, a11 + lam, a22 + lam
        b = [b[j] + lam * c[j] for j in range(3)]
        l10, l20 = a01 / a00, a02 / a00
        e1, t21 = a11 - l10 * a01, a12 - l20 * a01
        l21 = t21 / e1
        e2 = (a22 - l20 * a02) - l21 * t21
        z1 = b[1] - l10 * b[0]
        z2 = (b[2] - l20 * b[0]) - l21 * z1
        x2 = z2 / e2
        x1 = z1 / e1 - l21 * x2
        x0 = (b[0] / a00 - l10 * x1) - l20 * x2
        x = np.stack([np.where(lam > 0.0, y, cj) for y, cj in zip((x0, x1, x2), c)], axis=1)
        x = np.where(x >= -0.5, x, -0.5)
        x = np.where(x <= 0.5, x, 0.5)
    return x


def cluster_simplify(verts, faces, origin, pitch, cells, reg=0.05):
    """verts [V,3] float32, faces [F,3] integers of one image -> dict of verts_out [K,3] float32, faces_out [F',3] int32, vertex_cluster
    [V] int32, face_source [F'] int32, collapsed, cancelled (ints) and acc [K,13] int64.  ValueError("bad_vertex") / ("bad_index") where
    the kernel sets its flags."""
    assert 1 <= cells <= MAX_CELLS and np.float32(pitch) > 0 and np.isfinite(reg) and reg > 0
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V, G = len(verts), int(cells)
    q, cell, bad = locate(verts, origin, pitch, G)
    if bad.any():
        raise ValueError("bad_vertex")
    if len(faces) and (faces.min() < 0 or faces.max() >= V):
        raise ValueError("bad_index")
    cid = (cell[:, 0] * G + cell[:, 1]) * G + cell[:, 2]
    ids, vc = np.unique(cid, return_inverse=True)                   # clusters in ascending cell id
    vc = vc.reshape(-1)
    K = len(ids)
    gcell = np.stack([ids // (G * G), ids // G % G, ids % G], axis=1)
    acc = np.zeros((K, 13), np.int64)
    np.add.at(acc[:, 0], vc, 1)
    u = q - (cell.astype(np.float64) + 0.5)
    for j in range(3):
        np.add.at(acc[:, 1 + j], vc, np.rint(u[:, j] * SCALE).astype(np.int64))
    part = np.flatnonzero((faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2]))
    fa = faces[part]
    k = vc[fa] if len(fa) else np.zeros((0, 3), np.int64)           # [P,3] cluster numbers of the corners
    if len(fa):
        qa, qb, qc = q[fa[:, 0]], q[fa[:, 1]], q[fa[:, 2]]
        e1, e2 = qb - qa, qc - qa
        N = [e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]]
        A = [_fix(N[i] * N[j]) for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
        for r in range(3):
            new = np.ones(len(fa), bool)
            for earlier in range(r):
                new &= k[:, r] != k[:, earlier]
            g = cell[fa[:, r]].astype(np.float64)
            w = [qa[:, j] - (g[:, j] + 0.5) for j in range(3)]
            d = (N[0] * w[0] + N[1] * w[1]) + N[2] * w[2]
            for t in range(6):
                np.add.at(acc[:, 4 + t], k[new, r], A[t][new])
            for j in range(3):
                np.add.at(acc[:, 10 + j], k[new, r], _fix(N[j] * d)[new])
    x = solve(acc, reg)
    o = np.asarray(origin, np.float32).astype(np.float64)
    h = np.float64(np.float32(pitch))
    verts_out = (o + ((gcell.astype(np.float64) + 0.5) + x) * h).astype(np.float32)
    groups = {}                                                     # ascending triple -> [[even faces], [odd faces]]
    collapsed = 0
    for f, (a, b, c) in zip(part.tolist(), k.tolist()):
        if a == b or b == c or a == c:
            collapsed += 1
            continue
        lo, mid, hi = sorted((a, b, c))
        odd = (a, b, c) not in ((lo, mid, hi), (mid, hi, lo), (hi, lo, mid))
        groups.setdefault((lo, mid, hi), [[], []])[odd].append(f)
    keep = sorted(min(g[p]) for g in groups.values() for p in (0, 1) if len(g[p]) > len(g[1 - p]))
    faces_out = vc[faces[keep]].astype(np.int32).reshape(-1, 3)
    return dict(verts_out=verts_out, faces_out=faces_out, vertex_cluster=vc.astype(np.int32), face_source=np.asarray(keep, np.int32),
                collapsed=collapsed, cancelled=len(part) - collapsed - len(keep), acc=acc)


# ---- the marching-cubes shapes of the tests: 17^3 level grids, indexed -------------------------------------------------------------------
S = 17
CENTRE = (8.1, 7.9, 8.2)
GENUS = {"sphere": 0, "torus": 1, "cube": 0, "plate": 0}


def level(name):
    g = np.arange(S, dtype=np.float64)
    x, y, z = (a - c for a, c in zip(np.meshgrid(g, g, g, indexing="ij"), CENTRE))
    if name == "sphere":
        return (np.sqrt(x * x + y * y + z * z) - 5.3).astype(np.float32)
    if name == "torus":
        return (np.sqrt((np.sqrt(x * x + y * y) - 4.6) ** 2 + z * z) - 2.1).astype(np.float32)
    if name == "cube":
        return (np.maximum(np.maximum(np.abs(x), np.abs(y)), np.abs(z)) - 4.4).astype(np.float32)
    if name == "plate":
        # one grid point thick, 9 x 9 points wide: inside at z = 12 only, so its two sheets (z = 11.5 and 12.5) lie on either side of a
        # cell boundary at pitch 2, 3 and 4.  (A plate whose two sheets share a layer of cells folds onto itself and cancels to no face.)
        out = np.full((S, S, S), 0.5, np.float32)
        out[4:13, 4:13, 12] = -0.5
        return out
    raise KeyError(name)


_MESH = {}


def indexed(tris):
    """triangles [T,3,3] float32 -> (verts [V,3] float32, faces [T,3] int32): corners with the same bits become one vertex."""
    flat = np.ascontiguousarray(tris, np.float32).reshape(-1, 3)
    verts, inverse = np.unique(flat, axis=0, return_inverse=True)
    return verts.astype(np.float32), inverse.reshape(-1, 3).astype(np.int32)


def mc_mesh(name):
    """The indexed marching-cubes mesh (grid-index units) of the named level grid, by oracle/isosurface_ref.marching_cubes; once."""
    if name not in _MESH:
        root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
        if root not in sys.path:
            sys.path.insert(0, root)
        from oracle import isosurface_ref
        _MESH[name] = indexed(isosurface_ref.marching_cubes(level(name)))
    return _MESH[name]


def cells_for(pitch):
    """G = ceil((S - 1) / pitch): the box of the evaluation, origin 0."""
    return -(-(S - 1) // pitch)
