"""numpy restatement of sc_mesh_self_intersections (include/shapeclipper_hip.h): the filtered float64 orientation sign, the strict
segment-against-triangle rule and the rule of a pair of faces, operation by operation, vectorised over candidate pairs; the counts and
the per-face integers of ops.mesh_self_intersections from ALL pairs of an image whose closed fp32 boxes overlap (no grid, no early
exit: the plain definition).  Also the same predicate in exact rational arithmetic (fractions.Fraction), for the host test only."""
from fractions import Fraction

import numpy as np

TOL = np.float64(2.0 ** -49)
HUGE = np.float32(1.0e15)


def sign3(a, b, c, d):
    """a, b, c, d [..., 3] float32 -> [...] int8 in {-1, 0, 1}: the header's sign of d against the plane (a, b, c)."""
    a, b, c, d = (np.asarray(t, np.float32).astype(np.float64) for t in (a, b, c, d))
    with np.errstate(all="ignore"):
        ad, bd, cd = a - d, b - d, c - d
        m1, m2 = bd[..., 0] * cd[..., 1], bd[..., 1] * cd[..., 0]
        m3, m4 = cd[..., 0] * ad[..., 1], cd[..., 1] * ad[..., 0]
        m5, m6 = ad[..., 0] * bd[..., 1], ad[..., 1] * bd[..., 0]
        det = (ad[..., 2] * (m1 - m2) + bd[..., 2] * (m3 - m4)) + cd[..., 2] * (m5 - m6)
        perm = (((np.abs(m1) + np.abs(m2)) * np.abs(ad[..., 2]) + (np.abs(m3) + np.abs(m4)) * np.abs(bd[..., 2]))
                + (np.abs(m5) + np.abs(m6)) * np.abs(cd[..., 2]))
        zero = np.abs(det) <= TOL * perm
    return np.where(zero, 0, np.where(det > 0.0, 1, -1)).astype(np.int8)


def pierces(p, q, t):
    """p, q [n,3], t [n,3,3] (a triangle in its own corner order) -> [n] bool: the header's pierces(p, q; t0, t1, t2)."""
    sp, sq = sign3(t[:, 0], t[:, 1], t[:, 2], p), sign3(t[:, 0], t[:, 1], t[:, 2], q)
    s0, s1, s2 = sign3(p, q, t[:, 0], t[:, 1]), sign3(p, q, t[:, 1], t[:, 2]), sign3(p, q, t[:, 2], t[:, 0])
    return (sp.astype(np.int32) * sq == -1) & (s0 != 0) & (s0 == s1) & (s1 == s2)


def degenerate(faces):
    f = np.asarray(faces).reshape(-1, 3)
    return (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])


def pair_hits(verts, faces, A, B):
    """verts [V,3] float32, faces [F,3] of one image, A < B [n] face numbers, none of them degenerate -> (shared [n] int, hit [n] bool):
    the indices each pair shares and whether it is a hit; pairs that share two or three are never one."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    A, B = np.asarray(A, np.int64), np.asarray(B, np.int64)
    fa, fb = faces[A], faces[B]
    ta, tb = verts[fa], verts[fb]                                      # [n,3,3]
    eq = fa[:, :, None] == fb[:, None, :]                              # [n, corner of A, corner of B]
    shared = eq.sum(axis=(1, 2))
    hit = np.zeros(len(A), bool)
    none = np.flatnonzero(shared == 0)
    for e in range(3):
        hit[none] |= pierces(ta[none, e], ta[none, (e + 1) % 3], tb[none])
        hit[none] |= pierces(tb[none, e], tb[none, (e + 1) % 3], ta[none])
    one = np.flatnonzero(shared == 1)
    sa, sb = eq[one].any(axis=2).argmax(axis=1), eq[one].any(axis=1).argmax(axis=1)
    r = np.arange(len(one))
    hit[one] |= pierces(ta[one][r, (sa + 1) % 3], ta[one][r, (sa + 2) % 3], tb[one])
    hit[one] |= pierces(tb[one][r, (sb + 1) % 3], tb[one][r, (sb + 2) % 3], ta[one])
    return shared, hit


def box_pairs(verts, faces):
    """-> (A, B) int64 with A < B: every pair of faces that do not repeat an index whose closed fp32 boxes overlap, in ascending (A, B)."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(faces)
    if F == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    t = verts[faces]
    mn, mx = t.min(axis=1), t.max(axis=1)
    live = ~degenerate(faces)
    out_a, out_b = [], []
    for s in range(0, F, 512):
        e = min(F, s + 512)
        meet = live[s:e, None] & live[None, :]
        for k in range(3):
            meet &= (mn[s:e, None, k] <= mx[None, :, k]) & (mn[None, :, k] <= mx[s:e, None, k])
        meet &= np.arange(s, e)[:, None] < np.arange(F)[None, :]
        a, b = np.nonzero(meet)
        out_a.append(a + s)
        out_b.append(b)
    return np.concatenate(out_a).astype(np.int64), np.concatenate(out_b).astype(np.int64)


def image_self_intersections(verts, faces):
    """One image -> dict of pairs, pairs_vertex, box_pairs, faces_hit, degenerate (ints), hits, partner [F] int32 and hit_pairs [n,2].
    ValueError("bad_vertex") / ("bad_index") where the kernel sets its flags."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(faces)
    with np.errstate(all="ignore"):
        if not (np.abs(verts) < HUGE).all():
            raise ValueError("bad_vertex")
    if F and (faces.min() < 0 or faces.max() >= len(verts)):
        raise ValueError("bad_index")
    A, B = box_pairs(verts, faces)
    shared, hit = pair_hits(verts, faces, A, B)
    hits = np.zeros(F, np.int32)
    partner = np.full(F, np.iinfo(np.int32).max, np.int64)
    ha, hb = A[hit], B[hit]
    np.add.at(hits, ha, 1)
    np.add.at(hits, hb, 1)
    np.minimum.at(partner, ha, hb)
    np.minimum.at(partner, hb, ha)
    partner[hits == 0] = -1
    return dict(pairs=int(hit.sum()), pairs_vertex=int((hit & (shared == 1)).sum()), box_pairs=int((shared <= 1).sum()),
                faces_hit=int((hits > 0).sum()), degenerate=int(degenerate(faces).sum()), hits=hits, partner=partner.astype(np.int32),
                hit_pairs=np.stack([ha, hb], axis=1))


def self_intersections(verts, faces, v_count, f_count):
    """A packed batch -> dict of the fields of ops.MeshIntersections as numpy arrays (pairs, pairs_vertex, box_pairs int64; faces_hit,
    degenerate int32 [B]; hits, partner int32 [F])."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    v_off = np.concatenate([[0], np.cumsum(v_count)]).astype(np.int64)
    f_off = np.concatenate([[0], np.cumsum(f_count)]).astype(np.int64)
    per = [image_self_intersections(verts[v_off[b]:v_off[b + 1]], faces[f_off[b]:f_off[b + 1]]) for b in range(len(v_off) - 1)]
    out = {k: np.asarray([r[k] for r in per], np.int64) for k in ("pairs", "pairs_vertex", "box_pairs")}
    out.update({k: np.asarray([r[k] for r in per], np.int32) for k in ("faces_hit", "degenerate")})
    out.update({k: np.concatenate([r[k] for r in per] + [np.zeros(0, np.int32)]).astype(np.int32) for k in ("hits", "partner")})
    return out


def pack(meshes):
    """[(verts, faces), ...] -> (verts [V,3] float32, faces [F,3] int32, v_count, f_count int64)."""
    v = np.concatenate([np.asarray(m[0], np.float32).reshape(-1, 3) for m in meshes] + [np.zeros((0, 3), np.float32)])
    f = np.concatenate([np.asarray(m[1], np.int32).reshape(-1, 3) for m in meshes] + [np.zeros((0, 3), np.int32)])
    return (v.astype(np.float32), f.astype(np.int32), np.asarray([len(np.asarray(m[0]).reshape(-1, 3)) for m in meshes], np.int64),
            np.asarray([len(np.asarray(m[1]).reshape(-1, 3)) for m in meshes], np.int64))


# ---- exact arithmetic (the host test) -------------------------------------------------------------------------------------------------------
def exact_sign3(a, b, c, d):
    """The sign of the exact determinant of the fp32 coordinates."""
    a, b, c, d = ([Fraction(float(x)) for x in np.asarray(t, np.float32)] for t in (a, b, c, d))
    ad, bd, cd = ([x - y for x, y in zip(t, d)] for t in (a, b, c))
    det = (ad[2] * (bd[0] * cd[1] - bd[1] * cd[0]) + bd[2] * (cd[0] * ad[1] - cd[1] * ad[0])) + cd[2] * (ad[0] * bd[1] - ad[1] * bd[0])
    return (det > 0) - (det < 0)


def exact_pair(verts, fa, fb):
    """-> (hit, all_nonzero): the rule of a pair with exact signs, and whether every sign the plain definition looks at is non-zero."""
    signs = []

    def s(*args):
        signs.append(exact_sign3(*args))
        return signs[-1]

    def pierce(p, q, t):
        sp, sq = s(t[0], t[1], t[2], p), s(t[0], t[1], t[2], q)
        e = [s(p, q, t[0], t[1]), s(p, q, t[1], t[2]), s(p, q, t[2], t[0])]
        return sp * sq == -1 and e[0] != 0 and e[0] == e[1] == e[2]

    ta, tb = [verts[i] for i in fa], [verts[i] for i in fb]
    common = [(i, j) for i in range(3) for j in range(3) if fa[i] == fb[j]]
    if len(common) >= 2:
        return False, True
    if len(common) == 1:
        sa, sb = common[0]
        tests = [pierce(ta[(sa + 1) % 3], ta[(sa + 2) % 3], tb), pierce(tb[(sb + 1) % 3], tb[(sb + 2) % 3], ta)]
    else:
        tests = [pierce(ta[e], ta[(e + 1) % 3], tb) for e in range(3)] + [pierce(tb[e], tb[(e + 1) % 3], ta) for e in range(3)]
    return any(tests), all(x != 0 for x in signs)


# ---- the hand cases of the tests: name -> (pairs, pairs_vertex, degenerate) -------------------------------------------------------------
SQUARE = [[0, 0, 0], [4, 0, 0], [0, 4, 0]]


def hand_case(name):
    """(verts, faces) of a named hand case."""
    if name == "crossing":                      # a triangle standing in the first one's interior
        return SQUARE + [[1, 1, -1], [1, 1, 1], [1, 2, 1]], [[0, 1, 2], [3, 4, 5]]
    if name == "shared_vertex":                 # the second face hangs on vertex 0; its opposite edge passes through the first
        return SQUARE + [[1, 1, -1], [1, 2, 1]], [[0, 1, 2], [0, 3, 4]]
    if name == "vertex_on_face":                # a corner exactly in the plane, inside the triangle
        return SQUARE + [[1, 1, 0], [1, 1, 2], [2, 1, 2]], [[0, 1, 2], [3, 4, 5]]
    if name == "coplanar":                      # two overlapping triangles of one plane
        return SQUARE + [[1, 1, 0], [5, 1, 0], [1, 5, 0]], [[0, 1, 2], [3, 4, 5]]
    if name == "edge_through_edge":             # the edge (3, 4) passes through the edge (1, 2) of the first, at (2, 2, 0)
        return SQUARE + [[2, 2, -1], [2, 2, 1], [6, 6, 0]], [[0, 1, 2], [3, 4, 5]]
    if name == "duplicate":
        return SQUARE, [[0, 1, 2], [1, 2, 0], [0, 1, 2]]
    if name == "degenerate":                    # a face that repeats an index, through the first one
        return SQUARE + [[1, 1, -1], [1, 1, 1]], [[0, 1, 2], [3, 4, 3]]
    raise KeyError(name)


HAND = {"crossing": (1, 0, 0), "shared_vertex": (1, 1, 0), "vertex_on_face": (0, 0, 0), "coplanar": (0, 0, 0),
        "edge_through_edge": (0, 0, 0), "duplicate": (0, 0, 0), "degenerate": (0, 0, 1)}       # (pairs, pairs_vertex, degenerate)


# ---- the soups of the tests: 40 vertices, 60 faces, seeded -----------------------------------------------------------------------------
def soup(kind, seed=0, n_verts=40, n_faces=60):
    """kind "random": coordinates uniform in [0, 1) x 16; "lattice": integers 0..4; "half": multiples of 0.5 in 0..4 with 1e-6 jitter on a
    fifth of the coordinates.  Faces: three distinct vertices each."""
    rng = np.random.default_rng([seed, {"random": 1, "lattice": 2, "half": 3}[kind]])
    if kind == "random":
        v = rng.random((n_verts, 3)) * 16.0
    elif kind == "lattice":
        v = rng.integers(0, 5, (n_verts, 3)).astype(np.float64)
    else:
        v = rng.integers(0, 9, (n_verts, 3)) * 0.5
        v = v + np.where(rng.random((n_verts, 3)) < 0.2, rng.uniform(-1e-6, 1e-6, (n_verts, 3)), 0.0)
    f = np.stack([rng.choice(n_verts, 3, replace=False) for _ in range(n_faces)])
    return v.astype(np.float32), f.astype(np.int32)


def two_spheres():
    """The 17^3 marching-cubes sphere and a copy of itself shifted by (3.3, 0.7, 0.2), as ONE mesh: the second copy's faces follow."""
    import mesh_simplify_ref
    v, f = mesh_simplify_ref.mc_mesh("sphere")
    shift = np.asarray([3.3, 0.7, 0.2], np.float32)
    return np.concatenate([v, (v + shift).astype(np.float32)]).astype(np.float32), np.concatenate([f, f + len(v)]).astype(np.int32)
