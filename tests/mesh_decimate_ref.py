"""numpy restatement of sc_mesh_decimate_round and sc_mesh_decimate_compact (include/shapeclipper_hip.h) for ONE image: the edge table
(count, owner, omin, omax), the fixed vertices, the sorted rings, the vertex quadrics summed in ring order, the candidates (two faces, not
both ends fixed, the link condition, not the tetrahedron case), the regularised LDL^T target and its cost, the flip test, the independent
set by claims on closed neighbourhoods, the budget, the collapse and the final vertex compaction.  numpy's elementwise operations round
once each and never fuse, which is what the kernels are built to do; the sums run in the header's order.  The shapes are those of
tests/mesh_smooth_ref.py."""
import numpy as np

import mesh_smooth_ref as shapes
from mesh_subdivide_ref import edge_table

REG = 1e-3
MAX_ROUNDS = 1024
ROUND_INTS = ("faces_out", "selected", "collapsed", "candidates", "rejected_link", "rejected_flip", "fixed_vertices")
OCTA_V, OCTA_F = shapes.OCTA_V, shapes.OCTA_F
shape = shapes.shape
f64 = np.float64


def icosphere(levels=2):
    """The unit icosphere after `levels` midpoint subdivisions (20 * 4^levels faces), oriented outward; float32 positions."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, f64) / np.linalg.norm(p) for p in v]
    for _ in range(levels):
        mid, out = {}, []
        for a, b, c in f:
            m = []
            for p, q in ((a, b), (b, c), (c, a)):
                key = (min(p, q), max(p, q))
                if key not in mid:
                    mid[key] = len(v)
                    x = v[p] + v[q]
                    v.append(x / np.linalg.norm(x))
                m.append(mid[key])
            out += [(a, m[0], m[2]), (b, m[1], m[0]), (c, m[2], m[1]), (m[0], m[1], m[2])]
        f = out
    return np.array(v).astype(np.float32), np.array(f, np.int32)


def tet_and_octa():
    """A tetrahedron (vertices 0..3) and an octahedron (4..9) in one image: the tetrahedron case beside edges that do collapse."""
    import mesh_topology_ref as topo
    return (np.concatenate([topo.TET_V, OCTA_V + np.float32(4.0)]).astype(np.float32),
            np.concatenate([topo.TET_F, OCTA_F + 4]).astype(np.int32))


def _cross(e1, e2):
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)


def _dot(u, v):
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def _quadric_terms(x, v, u, w):
    """The ten terms of triangle (v, u, w) for vertex v: N N^T (00 01 02 11 12 22), N d (3), d^2 with N = (x_u - x_v) x (x_w - x_v),
    d = N . x_v."""
    p = x[v]
    N = _cross(x[u] - p, x[w] - p)
    d = _dot(N, p)
    return np.stack([N[:, 0] * N[:, 0], N[:, 0] * N[:, 1], N[:, 0] * N[:, 2], N[:, 1] * N[:, 1], N[:, 1] * N[:, 2], N[:, 2] * N[:, 2],
                     N[:, 0] * d, N[:, 1] * d, N[:, 2] * d, d * d], axis=1)


def _solve(A, m, reg):
    """x of (A + lam I) x = b + lam m, lam = reg trace(A), row by row; m where lam is not > 0 or x is not finite."""
    a00, a01, a02, a11, a12, a22, b0, b1, b2 = (A[:, k] for k in range(9))
    with np.errstate(all="ignore"):
        lam = f64(reg) * ((a00 + a11) + a22)
        d00, d11, d22 = a00 + lam, a11 + lam, a22 + lam
        r0, r1, r2 = b0 + lam * m[:, 0], b1 + lam * m[:, 1], b2 + lam * m[:, 2]
        l10, l20 = a01 / d00, a02 / d00
        e1, t21 = d11 - l10 * a01, a12 - l20 * a01
        l21 = t21 / e1
        e2 = (d22 - l20 * a02) - l21 * t21
        z1 = r1 - l10 * r0
        z2 = (r2 - l20 * r0) - l21 * z1
        x2 = z2 / e2
        x1 = z1 / e1 - l21 * x2
        x0 = (r0 / d00 - l10 * x1) - l20 * x2
    x = np.stack([x0, x1, x2], axis=1)
    ok = (lam > 0) & np.isfinite(x).all(axis=1)
    return np.where(ok[:, None], x, m)


def _cost(A, x):
    a00, a01, a02, a11, a12, a22, b0, b1, b2, c = (A[:, k] for k in range(10))
    x0, x1, x2 = x[:, 0], x[:, 1], x[:, 2]
    with np.errstate(all="ignore"):
        ax0 = (a00 * x0 + a01 * x1) + a02 * x2
        ax1 = (a01 * x0 + a11 * x1) + a12 * x2
        ax2 = (a02 * x0 + a12 * x1) + a22 * x2
        xax = (x0 * ax0 + x1 * ax1) + x2 * ax2
        bx = (b0 * x0 + b1 * x1) + b2 * x2
        cost = (xax - f64(2.0) * bx) + c
    return np.where(cost > 0, cost, f64(0.0))


def one_round(verts, faces, target, reg=REG, parent=None):
    """One round.  verts [V,3] float32 (every input vertex keeps its row), faces [F,3] integers of one image, target an integer ->
    dict of verts [V,3] float32, faces [F',3] int32, parent [V] (a removed vertex points at its survivor), fixed [V] bool (of THIS
    round's input), the ROUND_INTS, and for the tests `edges_selected` / `edges_collapsed`: lists of (a, b, key), `rings`: the closed
    neighbourhood sets of the selected edges.  ValueError("bad_vertex") / ("bad_index") / ("bad_face") where the kernel sets its flags."""
    verts = np.array(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V, F = len(verts), len(faces)
    parent = np.arange(V, dtype=np.int64) if parent is None else np.array(parent, np.int64)
    if not np.isfinite(verts).all():
        raise ValueError("bad_vertex")
    table = edge_table(faces, V)
    E = len(table)
    items = list(table.items())
    lo, hi, count, owner, omin, omax = (np.array([pick(e) for e in items], np.int64).reshape(E) for pick in (
        lambda e: e[0][0], lambda e: e[0][1], lambda e: e[1][0], lambda e: e[1][1], lambda e: e[1][2], lambda e: e[1][3]))
    fixed = np.zeros(V, bool)
    sharp = count != 2
    fixed[lo[sharp]] = True
    fixed[hi[sharp]] = True
    rows = [[] for _ in range(V)]
    for e, ((a, b), _) in enumerate(items):
        rows[a].append((b, e))
        rows[b].append((a, e))
    degree = np.array([len(r) for r in rows], np.int64).reshape(V)
    width = int(degree.max()) if V else 0
    nbr, eidx = np.zeros((V, width), np.int64), np.zeros((V, width), np.int64)
    for i, r in enumerate(rows):
        r.sort()
        nbr[i, :len(r)] = [t[0] for t in r]
        eidx[i, :len(r)] = [t[1] for t in r]
    x = verts.astype(f64)
    # vertex quadrics: ascending ring neighbour, then omin, omax of the edge slot
    Q = np.zeros((V, 10), f64)
    for k in range(width):
        v = np.flatnonzero(degree > k)
        u, e = nbr[v, k], eidx[v, k]
        Q[v] = Q[v] + _quadric_terms(x, v, u, omin[e])
        two = omax[e] != omin[e]
        v2 = v[two]
        Q[v2] = Q[v2] + _quadric_terms(x, v2, u[two], omax[e][two])
    # candidates
    ring = [set(t[0] for t in r) for r in rows]
    consider = (count == 2) & ~(fixed[lo] & fixed[hi])
    link = np.array([len(ring[a] & ring[b]) == 2 for a, b in zip(lo.tolist(), hi.tolist())], bool).reshape(E)
    cand = consider & link & ~((degree[lo] == 3) & (degree[hi] == 3))
    ce = np.flatnonzero(cand)
    a, b = lo[ce], hi[ce]
    A = Q[a] + Q[b]
    m = f64(0.5) * (x[a] + x[b])
    xt = _solve(A, m, reg)
    xt = np.where(fixed[a][:, None], x[a], np.where(fixed[b][:, None], x[b], xt))
    cost = _cost(A, xt)
    with np.errstate(all="ignore"):
        bits = cost.astype(np.float32).view(np.uint32).astype(np.uint64)
        target_f = xt.astype(np.float32)
    key = (bits << np.uint64(32)) | owner[ce].astype(np.uint64)
    tx = np.zeros((E, 3), f64)
    tx[ce] = target_f.astype(f64)
    # no flips: a thread per face corner walks the corner's ring
    valid = cand.copy()
    if F and width:
        fc = np.repeat(np.arange(F), 3)
        cc = np.tile(np.arange(3), F)
        v = faces[fc, cc]
        p, q = faces[fc, (cc + 1) % 3], faces[fc, (cc + 2) % 3]
        for k in range(width):
            u, e = nbr[v, k], eidx[v, k]
            on = (degree[v] > k) & ~fixed[v] & (u != p) & (u != q) & cand[e]
            if not on.any():
                continue
            f_, c_, e_ = fc[on], cc[on], e[on]
            P = x[faces[f_]]                                            # [n, 3 corners, 3]
            N = _cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
            P2 = P.copy()
            P2[np.arange(len(f_)), c_] = tx[e_]
            N2 = _cross(P2[:, 1] - P2[:, 0], P2[:, 2] - P2[:, 0])
            with np.errstate(all="ignore"):
                flip = ~(_dot(N2, N) > 0)
            valid[e_[flip]] = False
    rejected_flip = int(cand.sum() - valid.sum())
    # independent set: the 64-bit minimum of the keys on every vertex of the closed neighbourhood
    claim = {}
    pos = {int(e): i for i, e in enumerate(ce.tolist())}
    closed = {}
    for e in np.flatnonzero(valid).tolist():
        k = int(key[pos[e]])
        closed[e] = ring[int(lo[e])] | ring[int(hi[e])]                 # holds both ends
        for vtx in closed[e]:
            if k < claim.get(vtx, 1 << 64):
                claim[vtx] = k
    selected = sorted((int(key[pos[e]]), e) for e in closed if all(claim[vtx] == int(key[pos[e]]) for vtx in closed[e]))
    need = (F - target + 1) // 2 if F > target else 0
    go = selected[:need]
    out = verts.copy()
    for _, e in go:
        ea, eb = int(lo[e]), int(hi[e])
        s, r = (eb, ea) if (fixed[eb] and not fixed[ea]) else (ea, eb)
        if not fixed[s]:
            out[s] = target_f[pos[e]]
        parent[r] = s
    mapped = parent[faces] if F else faces
    keep = (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 1] != mapped[:, 2]) & (mapped[:, 2] != mapped[:, 0]) if F else np.zeros(0, bool)
    new_faces = mapped[keep].astype(np.int32).reshape(-1, 3)
    referenced = np.zeros(V, bool)
    referenced[faces.reshape(-1)] = True
    return dict(verts=out, faces=new_faces, parent=parent, fixed=fixed, faces_out=len(new_faces), selected=len(selected), collapsed=len(go),
                candidates=int(cand.sum()), rejected_link=int(consider.sum() - cand.sum()), rejected_flip=rejected_flip,
                fixed_vertices=int((fixed & referenced).sum()),
                edges_selected=[(int(lo[e]), int(hi[e]), k) for k, e in selected], edges_collapsed=[(int(lo[e]), int(hi[e]), k) for k, e in go],
                rings=[closed[e] for _, e in selected])


def compact(verts, faces, parent, fixed):
    """The vertices still referenced, in ascending input number -> (verts', faces', vertex_map [V], fixed')."""
    V = len(verts)
    used = np.zeros(V, bool)
    used[np.asarray(faces, np.int64).reshape(-1)] = True
    number = np.cumsum(used) - 1
    root = np.arange(V)
    for v in range(V):
        r = v
        while parent[r] != r:
            r = int(parent[r])
        root[v] = r
    vertex_map = np.where(used[root], number[root], -1).astype(np.int32)
    return verts[used], number[np.asarray(faces, np.int64)].astype(np.int32).reshape(-1, 3), vertex_map, fixed[used]


def decimate(verts, faces, target, reg=REG, max_rounds=MAX_ROUNDS, history=None):
    """Rounds until the image is at or below `target` faces, a round selects nothing, or max_rounds.  -> dict of verts [V',3] float32,
    faces [F',3] int32, vertex_map [V] int32, fixed [V'] bool (of the INPUT mesh), rounds, collapses, rejected_link, rejected_flip (sums
    over the rounds), fixed_vertices (of the input mesh), reached.  `history`, a list, receives every round's dict."""
    verts = np.array(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    first = one_round(verts, faces, max(len(faces), target), reg)       # the checks and the input's fixed vertices; collapses nothing
    fixed, parent = first["fixed"], first["parent"]
    rounds = collapses = rejected_link = rejected_flip = 0
    while len(faces) > target and rounds < max_rounds:
        r = one_round(verts, faces, target, reg, parent)
        if history is not None:
            history.append(r)
        rounds += 1
        collapses += r["collapsed"]
        rejected_link += r["rejected_link"]
        rejected_flip += r["rejected_flip"]
        verts, faces, parent = r["verts"], r["faces"], r["parent"]
        if r["selected"] == 0:
            break
    v_out, f_out, vertex_map, fixed_out = compact(verts, faces, parent, fixed)
    return dict(verts=v_out, faces=f_out, vertex_map=vertex_map, fixed=fixed_out, rounds=rounds, collapses=collapses,
                rejected_link=rejected_link, rejected_flip=rejected_flip, fixed_vertices=first["fixed_vertices"],
                reached=int(len(faces) <= target))
