"""numpy restatement of sc_mesh_subdivide and sc_mesh_project_step (include/shapeclipper_hip.h) for ONE image: the half-edges and their
edges (count, owner, omin, omax), the vertex classes, the float64 even and odd rules with one rounding per operation, the numbering by
ascending owner, the four output faces, the counts -- and the fp32 Newton step.  numpy's elementwise operations round once each and
never fuse, which is what the kernels are built to do.  The shapes are those of tests/mesh_smooth_ref.py."""
import numpy as np

import mesh_smooth_ref as shapes

INTS = ("vertices_out", "edges", "sharp_edges", "fixed_vertices", "isolated", "degree_max")
OCTA_V, OCTA_F = shapes.OCTA_V, shapes.OCTA_F
double_cone, shape = shapes.double_cone, shapes.shape


def edge_table(faces, V):
    """{(lo, hi): [count, owner, omin, omax]} over the half-edges 3 f + c.  ValueError("bad_index") for a face index outside [0, V),
    ValueError("bad_face") for a face that repeats an index."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(faces) and (faces.min() < 0 or faces.max() >= V):
        raise ValueError("bad_index")
    if len(faces) and ((faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 2] == faces[:, 0])).any():
        raise ValueError("bad_face")
    table = {}
    for f, face in enumerate(faces.tolist()):
        for c in range(3):
            a, b, opp = face[c], face[(c + 1) % 3], face[(c + 2) % 3]
            e = table.setdefault((min(a, b), max(a, b)), [0, 3 * f + c, opp, opp])
            e[0] += 1
            e[1], e[2], e[3] = min(e[1], 3 * f + c), min(e[2], opp), max(e[3], opp)
    return table


def mesh_subdivide(verts, faces):
    """One level.  verts [V,3] float32, faces [F,3] integers of one image -> dict of verts [V + E,3] float32, faces [4 F,3] int32, fixed
    [V + E] bool and the six INTS.  ValueError("bad_vertex") / ("bad_index") / ("bad_face") where the kernel sets its flags."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V, F = len(verts), len(faces)
    if not np.isfinite(verts).all():
        raise ValueError("bad_vertex")
    table = edge_table(faces, V)
    rows, fixed = [set() for _ in range(V)], np.zeros(V, bool)
    for (lo, hi), (count, _, _, _) in table.items():
        rows[lo].add(hi)
        rows[hi].add(lo)
        if count != 2:
            fixed[lo] = fixed[hi] = True
    degree = np.array([len(r) for r in rows], np.int64).reshape(V)
    x = verts.astype(np.float64)
    # even
    interior = (degree > 0) & ~fixed
    width = int(degree.max()) if V else 0
    nbr = np.zeros((V, width), np.int64)
    for i, r in enumerate(rows):
        nbr[i, :len(r)] = sorted(r)
    s = np.zeros_like(x)
    for k in range(width):
        has = degree > k
        s[has] = s[has] + x[nbr[has, k]]
    with np.errstate(all="ignore"):
        beta = np.where(degree == 3, np.float64(0.1875), np.float64(0.375) / degree.astype(np.float64))
    w = np.where(degree == 3, np.float64(0.4375), np.float64(0.625))
    own = w[:, None] * x
    with np.errstate(all="ignore"):
        ring = beta[:, None] * s
        even = own + ring
    out_even = verts.copy()
    out_even[interior] = even[interior].astype(np.float32)
    # odd, in ascending owner
    edges = sorted(table.items(), key=lambda kv: kv[1][1])
    E = len(edges)
    lo, hi, count, owner, omin, omax = (np.array([pick(e) for e in edges], np.int64).reshape(E) for pick in (
        lambda e: e[0][0], lambda e: e[0][1], lambda e: e[1][0], lambda e: e[1][1], lambda e: e[1][2], lambda e: e[1][3]))
    ends = x[lo] + x[hi]
    wings = x[omin] + x[omax]
    near = np.float64(0.375) * ends
    far = np.float64(0.125) * wings
    sharp = count != 2
    odd = np.where(sharp[:, None], np.float64(0.5) * ends, near + far).astype(np.float32)
    number = {int(h): V + r for r, h in enumerate(owner.tolist())}
    new_faces = np.zeros((4 * F, 3), np.int32)
    for f, face in enumerate(faces.tolist()):
        m = [number[table[(min(face[c], face[(c + 1) % 3]), max(face[c], face[(c + 1) % 3]))][1]] for c in range(3)]
        i = face
        new_faces[4 * f:4 * f + 4] = [[i[0], m[0], m[2]], [i[1], m[1], m[0]], [i[2], m[2], m[1]], [m[0], m[1], m[2]]]
    n_sharp = int(sharp.sum())
    return dict(verts=np.concatenate([out_even, odd.reshape(E, 3)]), faces=new_faces, fixed=np.concatenate([fixed, sharp]),
                vertices_out=V + E, edges=E, sharp_edges=n_sharp, fixed_vertices=int(fixed.sum()) + n_sharp,
                isolated=int((degree == 0).sum()), degree_max=int(degree.max()) if V else 0)


def subdivide_levels(verts, faces, levels):
    """`levels` levels, each level's fp32 output the next one's input -> the last level's dict."""
    out = dict(verts=np.asarray(verts, np.float32).reshape(-1, 3), faces=np.asarray(faces, np.int32).reshape(-1, 3))
    for _ in range(levels):
        out = mesh_subdivide(out["verts"], out["faces"])
    return out


def project_step(verts, sdf, grad, fixed, scale, max_step):
    """verts [V,3], sdf [V], grad [V,3] float32, fixed [V] bool -> verts' [V,3] float32, every operation an fp32 one rounded once."""
    f32 = np.float32
    v, f, g = np.asarray(verts, f32).reshape(-1, 3), np.asarray(sdf, f32).reshape(-1), np.asarray(grad, f32).reshape(-1, 3)
    fixed = np.asarray(fixed, bool).reshape(-1)
    scale, max_step = f32(scale), f32(max_step)
    with np.errstate(all="ignore"):
        g2 = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        keep = fixed | ~np.isfinite(f) | ~np.isfinite(g2) | (g2 < f32(1e-12))
        t = f / g2
        d = (t[:, None] * g) * scale
        l = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        keep = keep | ~np.isfinite(l)
        r = max_step / l
        d = np.where((l > max_step)[:, None], d * r[:, None], d)
        moved = v - d
    assert moved.dtype == np.float32
    return np.where(keep[:, None], v, moved)
