"""numpy restatement of sc_mesh_topology (include/shapeclipper_hip.h): the rules of ops.mesh_topology for ONE image, with dictionaries
and a plain union-find.  Area and volume use the header's order: chunks of CHUNK consecutive faces, a chunk's partial 0.0 plus its
terms in ascending face number, the image's sum 0.0 plus the partials in ascending chunk number; float64, one rounding per operation.
Also the hand-counted meshes the host and GPU tests share."""
import numpy as np

CHUNK = 256         # SC_MESH_TOPOLOGY_CHUNK
INT_FIELDS = ("vertices", "unreferenced_vertices", "faces", "degenerate_faces", "edges", "boundary_edges", "nonmanifold_edges",
              "inconsistent_edges", "components", "largest_component_faces", "nonmanifold_vertices", "euler", "genus")
FLAGS = ("watertight", "oriented", "manifold")


class _Sets:
    """A plain union-find over hashable items; the representative is the smallest item."""

    def __init__(self):
        self.parent = {}

    def add(self, x):
        self.parent.setdefault(x, x)

    def find(self, x):
        while self.parent[x] != x:
            x = self.parent[x]
        return x

    def unite(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.parent[max(a, b)] = min(a, b)


def face_terms(p0, p1, p2):
    """(area term, volume term) of one face from three float64 points, every operation rounded once."""
    e1, e2 = p1 - p0, p2 - p0
    nx = e1[1] * e2[2] - e1[2] * e2[1]
    ny = e1[2] * e2[0] - e1[0] * e2[2]
    nz = e1[0] * e2[1] - e1[1] * e2[0]
    area = np.sqrt((nx * nx + ny * ny) + nz * nz) * np.float64(0.5)
    cx = p1[1] * p2[2] - p1[2] * p2[1]
    cy = p1[2] * p2[0] - p1[0] * p2[2]
    cz = p1[0] * p2[1] - p1[1] * p2[0]
    volume = ((p0[0] * cx + p0[1] * cy) + p0[2] * cz) / np.float64(6.0)
    return area, volume


def mesh_topology(verts, faces):
    """verts [V,3] float32, faces [F,3] integers of one image -> dict of INT_FIELDS (ints), FLAGS (bools), area, volume (np.float64) and
    face_component [F] int32."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V, F = len(verts), len(faces)
    assert F == 0 or (faces.min() >= 0 and faces.max() < V)
    live = [f for f in range(F) if len(set(faces[f].tolist())) == 3]
    edges = {}                                          # (lo, hi) -> [count, fwd, minface]
    for f in live:
        for k in range(3):
            a, b = int(faces[f, k]), int(faces[f, (k + 1) % 3])
            e = edges.setdefault((min(a, b), max(a, b)), [0, 0, f])
            e[0] += 1
            e[1] += a < b
            e[2] = min(e[2], f)
    comp, corner = _Sets(), _Sets()
    for f in live:
        comp.add(f)
        for v in faces[f].tolist():
            corner.add((f, v))
    for f in live:
        for k in range(3):
            a, b = int(faces[f, k]), int(faces[f, (k + 1) % 3])
            m = edges[(min(a, b), max(a, b))][2]
            comp.unite(f, m)
            corner.unite((f, a), (m, a))
            corner.unite((f, b), (m, b))
    face_component = np.full(F, -1, np.int32)
    for f in live:
        face_component[f] = comp.find(f)
    roots, sizes = np.unique(face_component[face_component >= 0], return_counts=True)
    fans = {}
    for c in corner.parent:
        if corner.find(c) == c:
            fans[c[1]] = fans.get(c[1], 0) + 1
    referenced = set(int(v) for f in live for v in faces[f])
    out = dict(vertices=len(referenced), unreferenced_vertices=V - len(referenced), faces=len(live), degenerate_faces=F - len(live),
               edges=len(edges), boundary_edges=sum(e[0] == 1 for e in edges.values()),
               nonmanifold_edges=sum(e[0] >= 3 for e in edges.values()),
               inconsistent_edges=sum(e[0] == 2 and e[1] != 1 for e in edges.values()), components=len(roots),
               largest_component_faces=int(sizes.max()) if len(sizes) else 0, nonmanifold_vertices=sum(n > 1 for n in fans.values()))
    out["euler"] = out["vertices"] - out["edges"] + out["faces"]
    out["watertight"] = out["boundary_edges"] == 0 and out["nonmanifold_edges"] == 0
    out["oriented"] = out["inconsistent_edges"] == 0
    out["manifold"] = out["nonmanifold_edges"] == 0 and out["nonmanifold_vertices"] == 0
    ok = out["watertight"] and out["oriented"] and out["manifold"] and out["faces"] > 0
    out["genus"] = out["components"] - int(out["euler"] / 2) if ok else -1
    p = verts.astype(np.float64)
    area, volume = np.float64(0.0), np.float64(0.0)
    for first in range(0, F, CHUNK):
        pa, pv = np.float64(0.0), np.float64(0.0)
        for f in range(first, min(first + CHUNK, F)):
            ta, tv = face_terms(p[faces[f, 0]], p[faces[f, 1]], p[faces[f, 2]]) if face_component[f] >= 0 else (np.float64(0.0),) * 2
            pa, pv = pa + ta, pv + tv
        area, volume = area + pa, volume + pv
    out.update(area=area, volume=volume, face_component=face_component)
    return out


# ---- the hand-counted meshes -----------------------------------------------------------------------------------------------------------
TET_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
TET_F = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)          # the unit-corner tetrahedron, oriented outward

CUBE_V = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)       # vertex 4x + 2y + z


def _quad(a, b, c, d):
    return [[a, b, c], [a, c, d]]


# six squares, counter-clockwise seen from outside: x = 0, x = 1, y = 0, y = 1, z = 0, z = 1
CUBE_F = np.array(_quad(0, 1, 3, 2) + _quad(4, 6, 7, 5) + _quad(0, 4, 5, 1) + _quad(2, 3, 7, 6) + _quad(0, 2, 6, 4) + _quad(1, 5, 7, 3),
                  np.int32)


def torus(n=4, m=4, R=2.0, r=0.75):
    """An n x m torus of 2 n m triangles, oriented outward: vertex (i, j) -> i m + j."""
    v = np.zeros((n * m, 3), np.float32)
    f = []
    for i in range(n):
        for j in range(m):
            u, w = 2 * np.pi * i / n, 2 * np.pi * j / m
            v[i * m + j] = [(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)]
            a, b, c, d = i * m + j, ((i + 1) % n) * m + j, ((i + 1) % n) * m + (j + 1) % m, i * m + (j + 1) % m
            f += _quad(a, b, c, d)
    return v, np.array(f, np.int32)


def soup(n_faces=200, n_verts=12, seed=3):
    """A random soup: many multi-edges, duplicate faces and degenerate faces."""
    rng = np.random.RandomState(seed)
    return rng.uniform(-1, 1, (n_verts, 3)).astype(np.float32), rng.randint(0, n_verts, (n_faces, 3)).astype(np.int32)


def meshes():
    """name -> (verts, faces, expected subset of the result), in a fixed order."""
    tet = dict(vertices=4, edges=6, faces=4, euler=2, genus=0, watertight=True, oriented=True, manifold=True, components=1,
               boundary_edges=0, nonmanifold_edges=0, inconsistent_edges=0, nonmanifold_vertices=0, degenerate_faces=0,
               unreferenced_vertices=0, largest_component_faces=4)
    flipped = CUBE_F.copy()
    flipped[3] = flipped[3, ::-1]
    two_v = np.concatenate([TET_V, TET_V + 3])
    far = np.array([[5, 5, 5], [6, 5, 5], [5, 6, 5], [5, 5, 6]], np.float32)
    # two tetrahedra sharing the edge {0, 1}: the second one is 0, 1, 4, 5
    edge_f = np.concatenate([TET_F, np.array([[0, 4, 1], [0, 1, 5], [0, 5, 4], [1, 4, 5]], np.int32)])
    edge_v = np.concatenate([TET_V, np.array([[0, -1, 0], [0, 0, -1]], np.float32)])
    # two tetrahedra sharing vertex 0: the second one is 0, 4, 5, 6
    vert_f = np.concatenate([TET_F, np.array([[0, 5, 4], [0, 4, 6], [0, 6, 5], [4, 5, 6]], np.int32)])
    vert_v = np.concatenate([TET_V, -TET_V[1:]])
    tv, tf = torus()
    out = {
        "tetrahedron": (TET_V, TET_F, tet),
        "cube": (CUBE_V, CUBE_F, dict(vertices=8, edges=18, faces=12, euler=2, genus=0, watertight=True, oriented=True, manifold=True)),
        "cube_flipped": (CUBE_V, flipped, dict(inconsistent_edges=3, oriented=False, genus=-1, euler=2, watertight=True)),
        "cube_open": (CUBE_V, CUBE_F[:10], dict(faces=10, edges=17, boundary_edges=4, euler=1, watertight=False, genus=-1)),
        "tets_share_edge": (edge_v, edge_f, dict(vertices=6, edges=11, faces=8, nonmanifold_edges=1, components=1, euler=3, genus=-1,
                                                 watertight=False, manifold=False)),
        "tets_share_vertex": (vert_v, vert_f, dict(vertices=7, edges=12, faces=8, watertight=True, nonmanifold_vertices=1, components=2,
                                                   genus=-1, manifold=False)),
        "tets_disjoint": (two_v, np.concatenate([TET_F, TET_F + 4]), dict(components=2, euler=4, genus=0, largest_component_faces=4)),
        "torus": (tv, tf, dict(vertices=16, edges=48, faces=32, euler=0, genus=1, watertight=True, oriented=True, manifold=True)),
        "tet_degenerate": (np.concatenate([TET_V, far[:1]]), np.concatenate([TET_F, np.array([[1, 1, 2]], np.int32)]),
                           dict(tet, degenerate_faces=1, unreferenced_vertices=1)),
    }
    return out
