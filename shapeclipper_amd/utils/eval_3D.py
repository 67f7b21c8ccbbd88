"""Evaluation geometry: dense SDF grid -> surface points -> Chamfer / F-score.
Call surface of the reference's utils/eval_3D.py.

  * compute_level_grid: the whole (N+1)^3 grid of every image goes through the HIP SDF kernel in ONE
    launch (the reference loops over N+1 slabs of small launches, eval_3D.py:27-35).
  * chamfer_distance: chamfer_3D.forward (HIP; csrc/chamfer_grid.hip exact grid search, csrc/chamfer.hip all pairs), then sqrt
    as the reference.
  * marching cubes / mesh sampling are third-party in the reference (PyMCubes, trimesh; CPU threads).
    They are used when importable; otherwise the mesh comes from the device marching-cubes kernels (csrc/isosurface.hip: the
    same vertex set, one vertex per sign-changing grid edge) and is sampled area-uniformly like trimesh does -- see DESIGN.md,
    SURVEY 8f-2.  meshes_device gives the same surface as an indexed mesh (shared vertices) for the PLY dumps of the evaluation.
  * icp_metrics (`--eval.icp`): the same metrics after a similarity ICP of the prediction onto the ground truth (ops.icp_align,
    csrc/icp.hip around the Chamfer search), reported beside the raw ones.
  * normal_metrics (`--eval.normals`): normal consistency, the mean |cosine| between each point's normal and its nearest neighbour's in
    the other cloud, both ways: the SDF's own normals for the prediction, k-NN PCA normals (ops.point_normals,
    csrc/point_normals.hip) for the ground truth, paired by the indices of the Chamfer search already made.
  * mesh_metrics (`--eval.mesh_dist`): completeness as the exact distance from every ground-truth point to the predicted MESH
    (ops.point_mesh_distance, csrc/point_mesh.hip) instead of to its nearest sample, for the marching-cubes mesh and, with
    `--eval.dual_mesh`, for the dual-contouring one, reported beside the sample-based metrics.
  * emd_metrics (`--eval.emd`): the Earth Mover's Distance of `--eval.emd_points` points of the prediction and of the ground truth, the
    mean pair distance of the best one-to-one matching (ops.emd_match, csrc/emd3d.hip: a forward auction, one workgroup per image),
    reported beside Chamfer: the third number of the Pix3D benchmark table.
  * iou_metrics (`--eval.iou`): the volumetric IoU of the two clouds, each turned into a solid of `--eval.iou_res`^3 voxels the same way
    -- shell, closing, fill of what the exterior cannot reach (ops.voxel_solid, csrc/voxel_solid.hip: one workgroup per cloud, the whole
    flood in LDS) -- reported beside Chamfer: the first number of that table, in the clouds' own frame.
  * mesh_stats (`--eval.mesh_stats`): watertightness, manifoldness, orientation, components, genus, area and volume of the meshes that
    are written, from an edge table and two union-finds on the device (ops.mesh_topology, csrc/mesh_topology.hip).
  * meshes_dual (`--eval.dual_mesh`): the dual-contouring mesh of the same grid from the SDF gradients at the crossings
    (csrc/dual_contour.hip), which keeps corners and creases that marching cubes chamfers at the grid pitch.
  * meshes_simplified (`--eval.simplify=k`): the marching-cubes mesh decimated by vertex clustering in cells of k grid pitches with
    quadric placement (ops.mesh_cluster_simplify, csrc/mesh_simplify.hip), and what the smaller file costs in distance.
  * meshes_smoothed (`--mesh.smooth=n`): the marching-cubes mesh after n Taubin lambda|mu iterations of the umbrella operator
    (ops.mesh_smooth, csrc/mesh_smooth.hip): the same faces, the grid's staircase gone, the volume within about a per cent.
  * mesh_ambient_occlusion (`--mesh.ao`): ambient occlusion of the marching-cubes mesh baked from the level grid itself
    (ops.level_ambient_occlusion, csrc/level_ao.hip) -- per vertex, per atlas texel (mesh_ao_atlas) and in the mesh pictures (mesh_shade).
  * meshes_subdivided (`--mesh.subdivide=n`): the marching-cubes mesh after n levels of Loop subdivision (ops.mesh_subdivide,
    csrc/mesh_subdivide.hip), its new vertices put back on the network's zero set by mesh.subdivide_project clamped Newton steps
    (ops.mesh_project_step): four times the faces per level for about 1.5 network evaluations per input face and step.
  * meshes_decimated (`--mesh.decimate=F`): the marching-cubes mesh brought to F faces by quadric edge collapses (ops.mesh_decimate,
    csrc/mesh_decimate.hip): faces are spent where the surface bends, the rim that the grid face cuts stays where it is.
  * mesh_intersections (`--mesh.self_intersect`): does a written mesh pass through itself?  The pairs of faces that properly cross
    (ops.mesh_self_intersections, csrc/mesh_intersect.hip), for every mesh variant the run writes.
"""
from __future__ import annotations

import collections
import threading

import numpy as np
import torch

import chamfer_3D

from .. import ops, packing
from . import options

try:
    import mcubes
    import trimesh
    HAVE_MESHING = True
except Exception:  # pragma: no cover
    HAVE_MESHING = False


@torch.no_grad()
def get_dense_3D_grid(opt, var, N=None):
    B = len(var.idx)
    N = N or opt.eval.vox_res
    lo, hi = opt.eval.range
    g = torch.linspace(lo, hi, N + 1, device=opt.device)
    pts = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), dim=-1)
    return pts.repeat(B, 1, 1, 1, 1)


@torch.no_grad()
def compute_level_grid(opt, sdf_network, proj_latent_sdf, points_3D):
    B, N = points_3D.shape[0], points_3D.shape[1]
    flat = points_3D.reshape(-1, 3).contiguous()
    if getattr(sdf_network, "eager", False):        # architectures outside the HIP family: one x-slab at a time, as the reference (:21-38)
        from ..model import eager_path
        with torch.no_grad():
            slabs = [eager_path.sdf_mlp(sdf_network, points_3D[:, i].reshape(B, -1, 3), proj_latent_sdf)[..., 0].view(B, N, N) for i in range(N)]
        return torch.stack(slabs, dim=1)
    w_pack, cbias = sdf_network.packed(proj_latent_sdf)
    sdf, _, _ = ops.sdf_forward(flat, w_pack, cbias, N * N * N, symmetric=bool(sdf_network.force_symmetry),
                                want_grad=False, want_feat=False)
    return sdf.view(B, N, N, N)


@torch.no_grad()
def normalize_pc(pc):
    assert len(pc.shape) == 3
    centred = pc - pc.mean(dim=1, keepdim=True)
    # extents of x and y (reference utils/eval_3D.py:26-30), all axes in one max and one min reduction instead of four strided ones
    ext = centred.amax(dim=1) - centred.amin(dim=1)                     # [B, 3]
    scale = ext[:, :2].amax(dim=-1)[:, None, None]
    return centred / (scale + 1.e-7)


@torch.no_grad()
def normalize_pc_params(pc):
    """(centre [B,1,3], scale [B,1,1]) of normalize_pc, by exactly its expressions: (pc - centre) / (scale + 1e-7) has the bits of
    normalize_pc(pc), and the same map applied to other points (the vertices of the mesh the cloud was sampled from: mesh_metrics) puts
    them in the cloud's normalised frame."""
    assert len(pc.shape) == 3
    centre = pc.mean(dim=1, keepdim=True)
    centred = pc - centre
    ext = centred.amax(dim=1) - centred.amin(dim=1)                     # [B, 3]
    scale = ext[:, :2].amax(dim=-1)[:, None, None]
    return centre, scale


def _edge_crossing_points(level, lo, hi, num_points, rng):
    """Surface samples from sign changes along the three grid axes (fallback when PyMCubes is absent)."""
    S = level.shape[0]
    pts = []
    idx = np.stack(np.meshgrid(np.arange(S), np.arange(S), np.arange(S), indexing="ij"), -1).astype(np.float32)
    for ax in range(3):
        a = np.take(level, np.arange(S - 1), axis=ax)
        b = np.take(level, np.arange(1, S), axis=ax)
        cross = (a * b) < 0
        t = a[cross] / (a[cross] - b[cross])
        base = np.take(idx, np.arange(S - 1), axis=ax)[cross]
        base[:, ax] += t
        pts.append(base)
    pts = np.concatenate(pts, 0) if pts else np.zeros((0, 3), np.float32)
    if len(pts) == 0:
        return np.zeros([num_points, 3])
    pick = rng.randint(0, len(pts), num_points)
    return written_position(pts[pick], lo, hi, S)


@torch.no_grad()
def surface_points_device(level, lo, hi, num_points, seed=0, iso=0.0, method="cubes"):
    """level [B,S,S,S] on the GPU -> (points [B,num_points,3], tris list) sampled area-uniformly on the iso-surface.

    Device-side replacement of `mcubes.marching_cubes` + `trimesh.Trimesh.sample` (reference utils/eval_3D.py:123-153)
    when those packages are absent: triangles from the HIP marching-cubes kernels (csrc/isosurface.hip; the vertex set is the one
    PyMCubes produces, `method="tetrahedra"` selects the table-free variant of rounds 1-2), a
    triangle per sample drawn with probability proportional to its area, a uniform point inside it (the same scheme
    trimesh uses).  Vertices get the reference's 1/S rescale.  No D2H of the (N+1)^3 grid, no Python threads; seeded per
    call (the draws of image b depend on `seed` and b only)."""
    from .. import ops
    B, S = level.shape[0], level.shape[1]
    dev = level.device
    tris, per_image = ops.isosurface_triangles(level, iso, method=method)
    t_all = written_position(tris, lo, hi, S)
    ends = torch.cumsum(per_image, 0)                                   # host: triangles up to and including image b
    starts = ends - per_image
    meshes = [t_all[int(starts[b]):int(ends[b])] for b in range(B)]
    out = torch.zeros(B, num_points, 3, device=dev)
    if t_all.shape[0] == 0:
        return out, meshes                                              # the reference returns zeros for an empty mesh
    # all images at once: inverse-CDF draw over the concatenated triangle list -- image b's samples search its own segment of the
    # (float64) cumulative area, so no per-image loop, launch sequence or host synchronisation is left
    e1, e2 = t_all[:, 1] - t_all[:, 0], t_all[:, 2] - t_all[:, 0]
    cdf = torch.cumsum(torch.linalg.cross(e1, e2).norm(dim=1).double(), 0)
    cdf0 = torch.cat([cdf.new_zeros(1), cdf])                           # cdf0[k] = area of the first k triangles
    st, en = starts.to(dev), ends.to(dev)
    base, total = cdf0[st], cdf0[en] - cdf0[st]                         # [B]
    # image b draws from its own generator seeded seed + b: the sharded evaluation (one sample per call, seed = idx) and a batched one
    # (eval.batch_size > 1, seed = first idx) sample the SAME surface points for the same image (a single [B, N, 3] draw does not: the
    # device Philox stream assigns values per thread of the whole launch).  B small rand launches, still no host synchronisation.
    gen = torch.Generator(device=dev)
    u = torch.empty(B, num_points, 3, device=dev)
    for b in range(B):
        gen.manual_seed(seed + b)
        torch.rand(num_points, 3, device=dev, generator=gen, out=u[b])
    target = base[:, None] + u[..., 0].double() * total[:, None]
    pick = torch.searchsorted(cdf, target.reshape(-1), right=True).view(B, num_points)
    pick = torch.minimum(torch.maximum(pick, st[:, None]), (en - 1).clamp_min(0)[:, None])      # stays inside the image's segment
    uv = u[..., 1:]
    uv = torch.where(uv.sum(dim=-1, keepdim=True) > 1, 1 - uv, uv)
    pts = t_all[pick, 0] + uv[..., :1] * e1[pick] + uv[..., 1:] * e2[pick]
    ok = (total > 0) & (en > st)                                        # empty or zero-area meshes keep their zeros
    return torch.where(ok[:, None, None], pts, out), meshes


def sampled_position(v, lo, hi, S):
    """v in grid-index units -> where the level grid of S points per axis was sampled: where the surface is and the networks are asked."""
    return lo + v * ((hi - lo) / (S - 1))


def written_position(v, lo, hi, S):
    """v in grid-index units -> the reference's rescale, which every written mesh and the surface samples carry (see mesh_attributes)."""
    return v / S * (hi - lo) + lo


@torch.no_grad()
def meshes_device(level, lo, hi, iso=0.0):
    """level [B,S,S,S] on the GPU -> per-image list of (vertices [V,3] float32, faces [F,3] int32), both on the device, vertices in world
    units: the indexed marching-cubes mesh of ops.isosurface_mesh (the form `mcubes.marching_cubes` returns in the reference), rescaled
    with surface_points_device's expression, so its de-indexed triangles are exactly the surface the metrics were sampled from."""
    mesh = ops.isosurface_mesh(level, iso)
    return mesh.split(written_position(mesh.verts, lo, hi, level.shape[1]))


def _padded_vertex_queries(mesh, lo, hi, S):
    """The one-launch layout of the per-vertex network queries of a PackedMesh: (P, query [B P, 3]) with P = 16 ceil(max V_b / 16) rows
    per image, image b's vertices at rows [b P, b P + V_b), padding rows repeating the image's first vertex (mesh.padded_rows), at
    sampled_position.  (0, None) when no image has a vertex."""
    P, rows = mesh.padded_rows(16)
    if P == 0:
        return 0, None
    return P, sampled_position(mesh.verts[rows.reshape(-1)], lo, hi, S).contiguous()


def _colours_and_normals(sdf_network, rgb_network, proj_latent_sdf, proj_latent_rgb):
    """-> run(query, B, P): query [B P, 3] in the padded one-launch layout (P a multiple of 16 rows per image) -> (rgb [B P, 3] sigmoid
    colours, normal [B P, 3] unit SDF gradients), by one ops.sdf_forward with d sdf/dx and the feature and one ops.rgb_points_forward on
    weight images packed once here; architectures outside the compiled family (sdf_network.eager / rgb_network.eager) run the same
    steps on stock operators (model/eager_path.py)."""
    if sdf_network.eager or rgb_network.eager:
        from ..model import eager_path

        def run(query, B, P):
            _, feat, grad = eager_path.sdf_conditional_output(sdf_network, B, query, proj_latent_sdf, compute_grad=True)
            rgb = eager_path.rgb_mlp(rgb_network, query.view(B, P, 3), proj_latent_rgb, feat.detach().view(B, P, -1)).reshape(-1, 3)
            return rgb, torch.nn.functional.normalize(grad.detach(), dim=1, eps=1e-12)
        return run
    w_pack, cbias = sdf_network.packed(proj_latent_sdf)
    v_pack, dbias = rgb_network.packed(proj_latent_rgb)

    def run(query, B, P):
        _, grad, feat = ops.sdf_forward(query, w_pack, cbias, P, symmetric=bool(sdf_network.force_symmetry), want_grad=True, want_feat=True)
        return ops.rgb_points_forward(query, grad, feat, v_pack, dbias, P, symmetric=bool(rgb_network.force_symmetry))
    return run


@torch.no_grad()
def mesh_attributes(opt, sdf_network, rgb_network, proj_latent_sdf, proj_latent_rgb, level_vox):
    """level_vox [B,S,S,S] (compute_level_grid) -> per image (vertices [V,3] fp32, faces [F,3] int32, normals [V,3] fp32 unit,
    colours [V,3] uint8), on the device: the mesh of meshes_device, written the same way, with the predicted colour and the unit SDF
    normal of every vertex.

    Query positions: colours and normals are evaluated where the level grid was sampled, lo + v (hi - lo) / (S - 1) with v in grid-index
    units.  The written vertices keep the reference's v / S (hi - lo) + lo rescale (meshes_device), which moves each vertex toward the
    grid's lower corner by (p - lo) / S, p its true position -- up to (hi - lo) / S per axis, off the zero level set; querying there would
    colour the wrong point.

    One ops.sdf_forward (with d sdf/dx and the feature) and one ops.rgb_points_forward serve all images: image b's vertices sit at rows
    [b P, b P + V_b), P = 16 ceil(max V_b / 16), padding rows repeat the image's first vertex and are dropped.  Colours are
    trunc(clamp(c, 0, 1) * 255), the recipe of util_vis.dump_images.  Architectures outside the compiled family (sdf_network.eager) run
    the same steps on stock operators (model/eager_path.py)."""
    lo, hi = opt.eval.range
    B, S = level_vox.shape[0], level_vox.shape[1]
    dev = level_vox.device
    mesh = ops.isosurface_mesh(level_vox)
    written = mesh.split(written_position(mesh.verts, lo, hi, S))       # meshes_device's expression: the same bytes as {idx}_mesh.ply
    V = mesh.v_count.tolist()
    P, query = _padded_vertex_queries(mesh, lo, hi, S)
    if P == 0:
        empty = (torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev),
                 torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.uint8, device=dev))
        return [empty] * B
    rgb, normal = _colours_and_normals(sdf_network, rgb_network, proj_latent_sdf, proj_latent_rgb)(query, B, P)
    colours = (rgb.clamp(0, 1) * 255).to(torch.uint8)
    return [(*written[b], normal[b * P:b * P + V[b]], colours[b * P:b * P + V[b]]) for b in range(B)]


TEXTURE_SLAB = 1 << 20     # texels per launch of mesh_texture's network chain: the feature tile costs 256 B a texel
TexturedMesh = collections.namedtuple("TexturedMesh", ["vertices", "faces", "uv", "atlas", "normal_atlas", "stats"])


def texture_face_uv(n_faces, A, T, device=None):
    """OBJ texture coordinates [n_faces, 3, 2] fp32 of the chart corners of faces 0..n_faces-1 in an A x A atlas of T-texel cells
    (include/shapeclipper_hip.h states the layout): vt = ((X0 + pk.x + 0.5) / A, 1 - (Y0 + pk.y + 0.5) / A), exact in fp32."""
    n = A // T
    f = torch.arange(n_faces, device=device)
    c, h = f >> 1, f & 1
    corner = torch.tensor([[[0, 0], [T - 3, 0], [0, T - 3]], [[T - 1, T - 1], [2, T - 1], [T - 1, 2]]], device=device)[h]     # [F,3,2]
    origin = torch.stack([T * (c % n), T * (c // n)], dim=1)[:, None]
    p = (origin + corner).double() + 0.5
    return torch.stack([p[..., 0] / A, 1 - p[..., 1] / A], dim=-1).float()


@torch.no_grad()
def mesh_texture(opt, sdf_network, rgb_network, proj_latent_sdf, proj_latent_rgb, level_vox, slab=None):
    """level_vox [B,S,S,S] (compute_level_grid) -> per image TexturedMesh(vertices [V,3] fp32, faces [F,3] int32, uv [F,3,2] fp32,
    atlas uint8 [A,A,3], normal_atlas uint8 [A,A,3], stats), on the device: the mesh of meshes_device, written the same way (so an OBJ
    of it overlays {idx}_mesh.ply), with one triangular chart of eval.texture_texels = T texels per face in an A x A atlas
    (ops.texture_layout: one A for the batch, set by its largest mesh) that holds the predicted colour, and a second atlas that holds
    the unit SDF normal as (n + 1) / 2.  include/shapeclipper_hip.h states the layout; unused texels are (127, 127, 127).

    ops.texture_queries turns the texels of the atlas rows that hold a face into query points at the positions the level grid was
    sampled at (mesh_attributes' positions, not the written v / S rescale); one sdf_forward with gradient and feature and one
    rgb_points_forward per slab evaluate them (_colours_and_normals; the eager path for other architectures); ops.texture_pack
    quantises.  The chain runs in slabs of at most `slab` (default TEXTURE_SLAB = 2^20) texels per launch over the whole batch, a whole
    number of 16-point tiles per image each: every texel is evaluated on its own, so the slab size changes no bit.

    stats = dict(faces, atlas, rows, err_mean, err_max): the self-check.  Every face's centroid (b = 1/3 each) is evaluated by the
    network directly -- its queries ride behind the texels as one more padded block per image -- and compared with the bilinear look-up
    (ops.texture_sample) of the colour atlas at the centroid's texture coordinate, in 0..255 units, largest channel difference per
    face, mean and max over the faces: how well T texels resolve the colour field at hand.  An image without faces gets an all-127
    atlas of side 64, rows 0 and errors 0."""
    lo, hi = opt.eval.range
    T = options.texture_texels(opt, always=True)
    B, S = level_vox.shape[0], level_vox.shape[1]
    dev = level_vox.device
    mesh = ops.isosurface_mesh(level_vox)
    written = mesh.split(written_position(mesh.verts, lo, hi, S))       # meshes_device's expression: the same bytes as {idx}_mesh.ply
    v_start, f_start, F = mesh.starts()
    A, _, rows = ops.texture_layout(max(F, default=0), T)
    grey = torch.full((64, 64, 3), 127, dtype=torch.uint8, device=dev)
    blank = lambda b: TexturedMesh(*written[b], torch.zeros(0, 3, 2, device=dev), grey, grey,
                                   dict(faces=0, atlas=64, rows=0, err_mean=0.0, err_max=0.0))
    if rows == 0:
        return [blank(b) for b in range(B)]
    n_tex = rows * A
    Pc = 16 * ((max(F) + 15) // 16)                                     # the centroid block
    P = n_tex + Pc
    query, face_of_texel = ops.texture_queries(mesh.verts, mesh.faces, v_start, f_start, F, A, T, lo, hi, S, rows, extra=Pc)
    q = query.view(B, P, 3)
    for b, (v, f) in enumerate(mesh.split()):
        tri = v[f.long()]                                                              # [F_b,3,3] grid-index units
        q[b, n_tex:] = q[b, 0]                                                         # padding repeats the image's first texel
        q[b, n_tex:n_tex + F[b]] = sampled_position(tri.sum(dim=1) / 3, lo, hi, S)
    # the chain, slab by slab: rows [s, e) of every image's block are one padded launch of e - s points per image
    slab = TEXTURE_SLAB if slab is None else int(slab)
    step = max(16, (slab // B) // 16 * 16)
    chain = _colours_and_normals(sdf_network, rgb_network, proj_latent_sdf, proj_latent_rgb)
    if step >= P:
        rgb, normal = chain(query, B, P)
        rgb, normal = rgb.view(B, P, 3), normal.view(B, P, 3)
    else:
        rgb, normal = torch.empty(B, P, 3, device=dev), torch.empty(B, P, 3, device=dev)
        for s in range(0, P, step):
            e = min(s + step, P)
            c, m = chain(q[:, s:e].reshape(-1, 3).contiguous(), B, e - s)
            rgb[:, s:e], normal[:, s:e] = c.view(B, e - s, 3), m.view(B, e - s, 3)
    atlas, atlas_n = ops.texture_pack(rgb[:, :n_tex].reshape(-1, 3).contiguous(), normal[:, :n_tex].reshape(-1, 3).contiguous(),
                                      face_of_texel, A, rows)
    # self-check at the face centroids: the viewer's look-up against the network's colour there
    uv = [texture_face_uv(F[b], A, T, dev) for b in range(B)]
    image = torch.cat([torch.full((F[b],), b, dtype=torch.int32, device=dev) for b in range(B)])
    looked = ops.texture_sample(atlas, torch.cat([u.mean(dim=1) for u in uv]).contiguous(), image)
    direct = torch.cat([rgb[b, n_tex:n_tex + F[b]] for b in range(B)]).clamp(0, 1) * 255
    err = (looked - direct).abs().amax(dim=1).double()
    out = []
    for b in range(B):
        if F[b] == 0:
            out.append(blank(b))
            continue
        e = err[f_start[b]:f_start[b] + F[b]]
        out.append(TexturedMesh(*written[b], uv[b], atlas[b], atlas_n[b],
                                dict(faces=F[b], atlas=A, rows=rows, err_mean=float(e.mean()), err_max=float(e.max()))))
    return out


MESH_RENDER_NEAR = 0.05    # world units: a face with a vertex nearer to the camera plane is dropped (the cameras stand camera.dist ~ 5 away)
MeshRender = collections.namedtuple("MeshRender", ["rgb", "mask", "normal", "depth", "face", "bary", "stats"])


class MeshRenderSample:
    """What mesh_render_sample leaves in var.mesh_render (a plain object: an EasyDict would turn a tuple into a list)."""

    def __init__(self, render, faces, pixels, iou_input, iou_volume):
        self.render, self.faces, self.pixels, self.iou_input, self.iou_volume = render, faces, pixels, iou_input, iou_volume


@torch.no_grad()
def mesh_render(opt, level_vox, textured, pose, intr, H, W, large_pixels=None):
    """The textured mesh as an unlit viewer draws it: level_vox [B,S,S,S] (compute_level_grid), textured the batch's TexturedMesh list
    (mesh_texture of the same grid), pose [B,3,4] or [B,V,3,4] world-to-camera, intr [B,3,3] for opt.H x opt.W pixels -> MeshRender(rgb
    [B,V,H,W,3] in [0, 1], mask [B,V,H,W] (1 where a face covers the pixel centre), normal [B,V,H,W,3] in the (n + 1) / 2 encoding of
    the normal PNGs, depth [B,V,H,W] camera z (0 on a miss), face int32, bary, stats as ops.mesh_raster returns them), on the device.

    The mesh is that of ops.isosurface_mesh(level_vox) -- the same call, bits and face order as the atlas of mesh_texture -- drawn at the
    positions the level grid was sampled at, lo + v (hi - lo) / (S - 1): mesh_attributes' positions, where the surface is and where the
    texture was baked.  The written v / S rescale of {idx}_mesh.ply and the OBJ is NOT used: it shifts the shape by up to (hi - lo) / S,
    several pixels at 224 x 224.  One ops.mesh_raster call for all views (include/shapeclipper_hip.h states its arithmetic); then per
    pixel uv = (bary0 vt0 + bary1 vt1) + bary2 vt2 with vt the face's chart corners (texture_face_uv) and ops.texture_sample of the
    colour atlas and of the normal atlas, both / 255.  A miss is data.bgcolor in rgb and mid-grey (0.5) in normal.  For H x W other
    than opt.H x opt.W the intrinsics are diag(W / opt.W, H / opt.H, 1) @ intr.  camera.model: orthographic is not implemented."""
    if opt.camera.model != "perspective":
        raise NotImplementedError("camera.model: %s -- eval_3D.mesh_render rasterises perspective cameras only" % (opt.camera.model,))
    lo, hi = opt.eval.range
    B, S = level_vox.shape[0], level_vox.shape[1]
    dev = level_vox.device
    mesh = ops.isosurface_mesh(level_vox)
    world = sampled_position(mesh.verts, lo, hi, S).contiguous()           # mesh_attributes' positions
    v_start, f_start, F = mesh.starts()
    pose = pose.float()
    pose = (pose[:, None] if pose.dim() == 3 else pose).contiguous()
    intr = intr.float()
    if (int(H), int(W)) != (int(opt.H), int(opt.W)):
        intr = intr * torch.tensor([W / opt.W, H / opt.H, 1.0], device=intr.device).view(1, 3, 1)
    kw = {} if large_pixels is None else dict(large_pixels=large_pixels)
    r = ops.mesh_raster(world, mesh.faces, v_start, f_start, F, pose, intr.contiguous(), int(H), int(W), MESH_RENDER_NEAR, **kw)
    V = pose.shape[1]
    mask = r.face >= 0
    bg, grey = float(opt.data.bgcolor), 0.5
    if sum(F) == 0:
        rgb, normal = torch.full((B, V, H, W, 3), bg, device=dev), torch.full((B, V, H, W, 3), grey, device=dev)
        return MeshRender(rgb, mask.float(), normal, r.depth, r.face, r.bary, r.stats)
    assert all(m.faces.shape[0] == F[b] for b, m in enumerate(textured)), "the texture was baked for another mesh"
    A = max(m.atlas.shape[0] for b, m in enumerate(textured) if F[b])
    blank = torch.full((A, A, 3), 127, dtype=torch.uint8, device=dev)
    atlas = torch.stack([m.atlas if F[b] else blank for b, m in enumerate(textured)]).contiguous()
    atlas_n = torch.stack([m.normal_atlas if F[b] else blank for b, m in enumerate(textured)]).contiguous()
    vt = torch.cat([m.uv for m in textured])                               # [sum F, 3, 2], image after image
    first = torch.tensor(f_start, device=dev).view(B, 1, 1, 1)
    corner = vt[(r.face.clamp(min=0).long() + first).clamp(max=vt.shape[0] - 1).view(-1)]      # [N,3,2]; a miss reads some face, unused
    t = r.bary.view(-1, 3, 1) * corner
    uv = ((t[:, 0] + t[:, 1]) + t[:, 2]).contiguous()
    image = torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(V * H * W)
    covered = mask.view(B, V, H, W, 1)
    rgb = torch.where(covered, (ops.texture_sample(atlas, uv, image) / 255).view(B, V, H, W, 3), torch.full((), bg, device=dev))
    normal = torch.where(covered, (ops.texture_sample(atlas_n, uv, image) / 255).view(B, V, H, W, 3), torch.full((), grey, device=dev))
    return MeshRender(rgb, mask.float(), normal, r.depth, r.face, r.bary, r.stats)


def mask_iou(a, b):
    """Boolean masks [B, ...] -> [B] float64 intersection over union, from integer sums on the device; an empty union gives 1."""
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    inter, union = (a & b).sum(dim=1), (a | b).sum(dim=1)
    return torch.where(union == 0, torch.ones_like(union, dtype=torch.float64), inter.double() / union.clamp(min=1).double())


def mesh_depth_grey(opt, render, intr, scale_dist):
    """Renderer.surface_depth_grey's mapping for a MeshRender of opt.H x opt.W intrinsics `intr` [B,3,3]: [B,V,H,W] in [0, 1], (depth -
    near f) / (1.4 f) clamped, near = camera.dist scale_dist - 0.7 and f the camera z per unit length of the pixel's ray -- black at the
    near sample plane of the volume render, white at the far one and on a miss."""
    B, V, H, W = render.depth.shape
    k = intr.float() * torch.tensor([W / opt.W, H / opt.H, 1.0], device=intr.device).view(1, 3, 1)
    x = (torch.arange(W, device=intr.device).float() + 0.5).view(1, 1, W)
    y = (torch.arange(H, device=intr.device).float() + 0.5).view(1, H, 1)
    dx, dy = (x - k[:, 0, 2].view(B, 1, 1)) / k[:, 0, 0].view(B, 1, 1), (y - k[:, 1, 2].view(B, 1, 1)) / k[:, 1, 1].view(B, 1, 1)
    fac = (1.0 / torch.sqrt(dx * dx + dy * dy + 1.0)).view(B, 1, H, W)
    near = (float(opt.camera.dist) * scale_dist.float() - 0.7).view(B, 1, 1, 1)
    grey = ((render.depth - near * fac) / (1.4 * fac)).clamp(0, 1)
    return torch.where(render.mask > 0, grey, torch.ones_like(grey))


@torch.no_grad()
def mesh_render_sample(opt, var, textured):
    """`--eval.mesh_render` for an evaluated batch: the textured mesh from the samples' own cameras (var.pose, var.intr) ->
    MeshRenderSample(render: the MeshRender at the size of var.mask_input_map (opt.H x opt.W without that map), faces [B] and pixels [B] (covered
    pixel centres of that render) as host lists, iou_input [B] float64: the mesh mask against var.mask_input_map >= 0.5 at that map's
    size, iou_volume [B] float64: a second rasterisation at opt.H x opt.W against var.mask_hard_map >= 0.5 -- integer sums on the
    device, an empty union gives 1, a missing map nan)."""
    B = len(var.idx)
    nan = torch.full((B,), float("nan"), dtype=torch.float64, device=var.level_vox.device)
    has_input = "mask_input_map" in var and var.mask_input_map is not None
    H, W = (int(s) for s in var.mask_input_map.shape[-2:]) if has_input else (int(opt.H), int(opt.W))
    render = mesh_render(opt, var.level_vox, textured, var.pose, var.intr, H, W)
    mask = render.mask[:, 0] > 0
    iou_input = mask_iou(mask, var.mask_input_map.reshape(B, H, W) >= 0.5) if has_input else nan
    iou_volume = nan
    if "mask_hard_map" in var and var.mask_hard_map is not None:
        at_render = render if (H, W) == (int(opt.H), int(opt.W)) else mesh_render(opt, var.level_vox, textured, var.pose, var.intr,
                                                                                    int(opt.H), int(opt.W))
        iou_volume = mask_iou(at_render.mask[:, 0] > 0, var.mask_hard_map.reshape(B, int(opt.H), int(opt.W)) >= 0.5)
    return MeshRenderSample(render, [int(m.faces.shape[0]) for m in textured], mask.reshape(B, -1).sum(dim=1).tolist(), iou_input, iou_volume)


@torch.no_grad()
def meshes_dual(opt, sdf_network, proj_latent_sdf, level_vox, reg, keep=None):
    """level_vox [B,S,S,S] (compute_level_grid) -> per image (vertices [Vd,3] fp32, faces [Fd,3] int32) on the device: the dual-contouring
    mesh of ops.dual_contour_mesh (`--eval.dual_mesh`, {idx}_mesh_dual.ply), which puts one vertex INSIDE every surface cell, where the
    tangent planes of the cell's crossings meet, so corners and creases narrower than the grid pitch survive; `reg` holds the vertex near
    the mean of the crossings.

    The normals are the unit SDF gradients at the crossing vertices of ops.isosurface_mesh, queried at mesh_attributes' positions in its
    padded one-launch layout (one ops.sdf_forward with d sdf/dx; sdf_network.eager: stock operators, model/eager_path.py).  The written
    vertices take meshes_device's v / S (hi - lo) + lo, so the mesh overlays {idx}_mesh.ply.  The crossing vertices are extracted twice,
    here for the queries and again inside dual_contour_mesh, whose public form takes the grid and the normals.  keep (the batch's var):
    keep.mesh_dual_packed = the PackedMesh as ops.dual_contour_mesh returned it (a list of its four fields), when there is a mesh."""
    lo, hi = opt.eval.range
    B, S = level_vox.shape[0], level_vox.shape[1]
    dev = level_vox.device
    mesh = ops.isosurface_mesh(level_vox)
    P, query = _padded_vertex_queries(mesh, lo, hi, S)
    if P == 0:
        return [(torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev))] * B
    if sdf_network.eager:
        from ..model import eager_path
        _, _, grad = eager_path.sdf_conditional_output(sdf_network, B, query, proj_latent_sdf, compute_grad=True)
    else:
        w_pack, cbias = sdf_network.packed(proj_latent_sdf)
        _, grad, _ = ops.sdf_forward(query, w_pack, cbias, P, symmetric=bool(sdf_network.force_symmetry), want_grad=True, want_feat=False)
    normal = torch.nn.functional.normalize(grad.detach(), dim=1, eps=1e-12)
    normals = torch.cat([normal[b * P:b * P + n] for b, n in enumerate(mesh.v_count.tolist())])
    dual = ops.dual_contour_mesh(level_vox, normals, 0.0, reg)
    if keep is not None:                    # the packed mesh in grid-index units, for mesh_stats
        keep.mesh_dual_packed = list(dual)
    return dual.split(written_position(dual.verts, lo, hi, S))


def convert_to_explicit_worker(opt, i, level_vox_i, isoval, meshes, pointclouds=None):
    lo, hi = opt.eval.range
    S = level_vox_i.shape[0]
    assert level_vox_i.shape[0] == level_vox_i.shape[1] == level_vox_i.shape[2]
    if HAVE_MESHING:
        vertices, faces = mcubes.marching_cubes(level_vox_i, isovalue=isoval)
        mesh = trimesh.Trimesh(written_position(vertices, lo, hi, S), faces)
        meshes[i] = mesh
        if pointclouds is not None:
            pointclouds[i] = mesh.sample(opt.eval.num_points) if len(mesh.triangles) != 0 else np.zeros([opt.eval.num_points, 3])
    else:
        meshes[i] = None
        if pointclouds is not None:
            pointclouds[i] = _edge_crossing_points(level_vox_i - isoval, lo, hi, opt.eval.num_points, np.random.RandomState(i))


def convert_to_explicit(opt, level_grids, isoval=0., to_pointcloud=False):
    n = len(level_grids)
    meshes = [None] * n
    pcs = [None] * n if to_pointcloud else None
    threads = [threading.Thread(target=convert_to_explicit_worker, args=(opt, i, level_grids[i], isoval, meshes),
                                kwargs=dict(pointclouds=pcs), daemon=False) for i in range(n)]
    for t in threads: t.start()
    for t in threads: t.join()
    return (meshes, np.stack(pcs, axis=0)) if to_pointcloud else meshes


def chamfer_distance(opt, X1, X2):
    B, N1, N2 = len(X1), X1.shape[1], X2.shape[1]
    assert X1.shape[2] == 3
    dev = X1.device
    d1 = torch.zeros(B, N1, device=dev); d2 = torch.zeros(B, N2, device=dev)
    i1 = torch.zeros(B, N1, dtype=torch.int32, device=dev); i2 = torch.zeros(B, N2, dtype=torch.int32, device=dev)
    chamfer_3D.forward(X1.contiguous().float(), X2.contiguous().float(), d1, d2, i1, i2)
    return d1.sqrt(), d2.sqrt(), i1, i2


def compute_fscore(dist1, dist2, thresholds=[0.005, 0.01, 0.02, 0.05, 0.1, 0.2]):
    # all thresholds at once (the reference loops over them, utils/eval_3D.py:160-167): the means are counts of exact 0 / 1 values
    # divided by N, so the result does not depend on how the reduction is grouped
    th = torch.tensor(list(thresholds), device=dist1.device, dtype=dist1.dtype)
    precision = (dist1[:, :, None] < th).float().mean(dim=1)            # [B, T]
    recall = (dist2[:, :, None] < th).float().mean(dim=1)
    f = 2 * precision * recall / (precision + recall)
    return torch.where(torch.isnan(f), torch.zeros_like(f), f)


def largest_component_enabled(opt):
    """`--hip.largest_component` (default off): eval_metrics keeps only the largest 6-connected component of the solid {level < 0}
    (ops.level_largest_component) -- var.level_vox is the filtered grid, var.component_stats the per-image counts -- so the metrics,
    the mesh and point-cloud dumps and the training-time visualisation all see the solid without its detached floaters."""
    return bool(options.hip(opt, "largest_component"))


@torch.no_grad()
def icp_metrics(opt, var, iters, scale):
    """`--eval.icp`: the metrics once more after ops.icp_align has registered the normalised prediction var.dpc_pred onto the normalised
    ground truth var.dpc.points -- what is left when normalize_pc's centring, scaling and a small residual rotation no longer count.
    Sets var.dpc_pred_icp (the aligned prediction), var.cd_acc_icp / var.cd_comp_icp [B] and var.f_score_icp [B,T], all from the square
    roots of the distances of the loop's LAST search (no further search), and var.icp = dict(transform [B,4,4], s [B], objective
    [B, iters+1]), float64.  The raw metrics are untouched.  A one-point prediction (an empty mesh) has no rotation to fit: its transform
    stays the identity and the numbers equal the raw ones.  Returns the IcpResult (normal_metrics pairs normals by its last search)."""
    res = ops.icp_align(var.dpc_pred.contiguous().float(), var.dpc.points.contiguous().float(), iters=iters, scale=scale)
    dist_acc, dist_comp = res.dist1.sqrt(), res.dist2.sqrt()
    var.dpc_pred_icp = res.aligned
    var.f_score_icp = compute_fscore(dist_acc, dist_comp, opt.eval.f_thresholds)
    var.cd_acc_icp = dist_acc.mean(dim=1)
    var.cd_comp_icp = dist_comp.mean(dim=1)
    var.icp = dict(transform=res.transform, s=res.s, objective=res.objective)
    return res


@torch.no_grad()
def predicted_normals(opt, sdf_network, proj_latent_sdf, points, S):
    """points [B,N,3] sampled on the written surface of an S^3 level grid, in the object frame -> [B,N,3] fp32 unit normals of the SDF
    there.  The sampled points carry the reference's v / S rescale (surface_points_device, convert_to_explicit_worker), which moves a
    point p toward the grid's lower corner by (p - lo) / S (mesh_attributes); the network is asked where the grid was sampled,
    lo + (p - lo) S / (S - 1).  One ops.sdf_forward with d sdf/dx for all images: P = 16 ceil(N / 16) rows per image, padding rows
    repeat the image's first point and are dropped (_padded_vertex_queries' layout).  sdf_network.eager: stock operators."""
    lo, hi = opt.eval.range
    B, N = points.shape[0], points.shape[1]
    q = lo + (points.float() - lo) * (S / (S - 1))
    P = 16 * ((N + 15) // 16)
    query = torch.cat([q, q[:, :1].expand(B, P - N, 3)], dim=1).reshape(-1, 3).contiguous()
    if getattr(sdf_network, "eager", False):
        from ..model import eager_path
        _, _, grad = eager_path.sdf_conditional_output(sdf_network, B, query, proj_latent_sdf, compute_grad=True)
    else:
        w_pack, cbias = sdf_network.packed(proj_latent_sdf)
        _, grad, _ = ops.sdf_forward(query, w_pack, cbias, P, symmetric=bool(sdf_network.force_symmetry), want_grad=True, want_feat=False)
    normal = torch.nn.functional.normalize(grad.detach().float(), dim=1, eps=1e-12)
    return normal.view(B, P, 3)[:, :N].contiguous()


@torch.no_grad()
def normal_metrics(opt, var, sdf_network, points_object, idx1, idx2, k, icp=None):
    """`--eval.normals`: normal consistency beside the raw metrics.  points_object [B,N,3] are the prediction's samples in the object
    frame, before eval_metrics moved them; idx1 [B,N] / idx2 [B,M] the nearest-neighbour indices of the raw Chamfer search between
    var.dpc_pred and var.dpc.points (no further search).
      prediction: predicted_normals at points_object, then the orthogonal maps the points went through -- var.pose[..., :3] and, for
        Pix3D, the flip; normalize_pc is a translation and a uniform scale and leaves normals alone.  -> var.normals_pred [B,N,3].
      ground truth: ops.point_normals(var.dpc.points, k) on the normalised cloud: PCA normals, ESTIMATED from the points (the processed
        ground truth has none) and unoriented, hence the absolute cosine.  -> var.dpc.normals (the slot the loader leaves at zero) and
        var.dpc.variation.
    Sets var.nc_acc, var.nc_comp (ops.normal_consistency) and var.nc = (nc_acc + nc_comp) / 2, [B] float64.  With `icp` (the IcpResult
    of icp_metrics): var.nc_acc_icp / nc_comp_icp / nc_icp from the last ICP search's indices, the predicted normals rotated by
    transform[:, :3, :3] / s (var.normals_pred_icp)."""
    dev = var.idx.device
    B = points_object.shape[0]
    rot = lambda Rm, P: (Rm @ P.permute(0, 2, 1)).permute(0, 2, 1).contiguous()
    normals = predicted_normals(opt, sdf_network, var.proj_latent_sdf, points_object, var.level_vox.shape[1])
    normals = rot(var.pose[..., :3].float(), normals)
    if opt.data.dataset in ["pix3d"]:
        normals = rot(torch.tensor(_FLIP_PRED).float().to(dev).unsqueeze(0).expand(B, 3, 3), normals)
    gt = ops.point_normals(var.dpc.points.contiguous().float(), k)
    var.normals_pred = normals
    var.dpc.normals, var.dpc.variation = gt.normals, gt.variation
    var.nc_acc, var.nc_comp = ops.normal_consistency(normals, gt.normals, idx1.contiguous(), idx2.contiguous())
    var.nc = (var.nc_acc + var.nc_comp) / 2
    if icp is not None:
        R = icp.transform[:, :3, :3] / icp.s[:, None, None]
        var.normals_pred_icp = rot(R, normals.double()).float()
        var.nc_acc_icp, var.nc_comp_icp = ops.normal_consistency(var.normals_pred_icp, gt.normals, icp.idx1, icp.idx2)
        var.nc_icp = (var.nc_acc_icp + var.nc_comp_icp) / 2


def _pack_meshes(meshes, anchors):
    """[(verts [V,3], faces [F,3] int32)] per image -> their ops.PackedMesh (host counts).  An image with an empty mesh is given ONE
    degenerate triangle, three times anchors[b] (anchors [B,3]: a point per image)."""
    dev = anchors.device
    verts, faces, nv, nf = [], [], [], []
    for b, (v, f) in enumerate(meshes):
        if f.shape[0] == 0 or v.shape[0] == 0:
            v, f = anchors[b:b + 1].float().expand(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32, device=dev)
        verts.append(v.float()); faces.append(f.to(torch.int32)); nv.append(v.shape[0]); nf.append(f.shape[0])
    return ops.PackedMesh(torch.cat(verts).contiguous(), torch.cat(faces).contiguous(), torch.tensor(nv, dtype=torch.int64),
                          torch.tensor(nf, dtype=torch.int64))


@torch.no_grad()
def mesh_metrics(opt, var, sdf_network, frame):
    """`--eval.mesh_dist`: completeness against the predicted SURFACE instead of against samples of it.  The sample-based completeness
    is the distance from a ground-truth point to the nearest of eval.num_points samples, which has a floor of about the sample spacing
    (0.005 at 100,000 samples, the finest F-score threshold) and a seed-dependent jitter of that size; the exact distance to the mesh
    (ops.point_mesh_distance) has neither, and works for any mesh.

    The mesh is meshes_device(var.level_vox, lo, hi) -- also when PyMCubes is importable: the vertex set is the same -- with the v / S
    rescale the samples carry.  Its vertices go through the maps the samples went through: var.pose[..., :3], the Pix3D flip, then
    `frame` = (centre, scale) of normalize_pc_params of the SAMPLES, which eval_metrics captured before it normalised var.dpc_pred; a
    sample lies on the mesh, so after the same maps it still does.  An image with an empty mesh gets one degenerate triangle at
    var.dpc_pred[b, 0], so its numbers equal the sample-based ones (the convention of --eval.icp for an empty mesh).
    Sets var.dist_comp_mesh [B,M] (the square root of the kernel's squared distance), var.cd_comp_mesh [B], var.face_mesh [B,M] int32
    and var.f_score_mesh [B,T] = compute_fscore(precision from the sample-based var.dist_acc, recall from the mesh distances).  With
    `--eval.dual_mesh`: the same for the mesh of meshes_dual -> var.dist_comp_dual, var.cd_comp_dual, var.f_score_dual, var.face_dual;
    that mesh stays in var.mesh_dual (object frame) for the dump.  The accuracy direction stays sample-based (the ground truth is a
    bare point cloud), nothing is ICP-aligned, nothing enters a loss."""
    lo, hi = opt.eval.range
    dev = var.idx.device
    centre, scale = frame
    gt = var.dpc.points.contiguous().float()
    rot = lambda Rm, P: (Rm @ P.t()).t()

    def to_frame(meshes):
        out = []
        for b, (v, f) in enumerate(meshes):
            v = rot(var.pose[b, :, :3].float(), v.float())
            if opt.data.dataset in ["pix3d"]:
                v = rot(torch.tensor(_FLIP_PRED).float().to(dev), v)
            out.append((((v - centre[b]) / (scale[b] + 1.e-7)).contiguous(), f))
        return out

    def measure(meshes, suffix):
        res = ops.point_mesh_distance(gt, *_pack_meshes(to_frame(meshes), var.dpc_pred[:, 0]), search="grid")
        dist = res.dist2.sqrt()
        var["dist_comp_" + suffix] = dist
        var["cd_comp_" + suffix] = dist.mean(dim=1)
        var["face_" + suffix] = res.face
        var["f_score_" + suffix] = compute_fscore(var.dist_acc, dist, opt.eval.f_thresholds)

    measure(meshes_device(var.level_vox, lo, hi), "mesh")
    reg = options.dual_mesh_reg(opt)
    if reg is not None:
        var.mesh_dual = meshes_dual(opt, sdf_network, var.proj_latent_sdf, var.level_vox, reg, keep=var)
        measure(var.mesh_dual, "dual")


def emd_subsample(pred, gt, points):
    """(pred[:, :n], gt[:, floor(k M / n)], n) with n = min(points, N, M): the two n-point clouds emd_metrics matches.  The surface
    samples are independent draws, so a prefix of them is a uniform sub-sample; the ground truth may be stored in any order, so it is
    taken at an even stride over all of its M rows."""
    N, M = pred.shape[1], gt.shape[1]
    n = min(points, N, M)
    rows = torch.arange(n, device=gt.device, dtype=torch.int64) * M // n
    return pred[:, :n].contiguous().float(), gt[:, rows].contiguous().float(), n


@torch.no_grad()
def emd_metrics(opt, var, points, eps, icp=None):
    """`--eval.emd`: the Earth Mover's Distance between emd_subsample's n points of the normalised prediction var.dpc_pred and of the
    normalised ground truth var.dpc.points -- the mean distance of the pairs of a one-to-one matching that is within `eps` of the
    cheapest (ops.emd_match), so, unlike Chamfer, it charges for mass in the wrong place.  Sets var.emd [B] float64, var.emd_n (the
    int n), var.emd_rounds / var.emd_converged [B] int32 and var.emd_assignment [B,n] int32 (the ground-truth row of every predicted
    point, in the sub-samples' numbering).  With `--eval.icp` (icp = icp_metrics' result): the same for the first n rows of
    var.dpc_pred_icp -> var.emd_icp, var.emd_rounds_icp, var.emd_converged_icp, var.emd_assignment_icp.  The clouds are normalised to
    unit extent, which the auction's first epsilon of 0.25 is sized for.  An empty mesh is n coincident points, like any cloud.  The
    raw metrics are untouched, nothing enters a loss."""
    gt = var.dpc.points
    for suffix, pred in (("", var.dpc_pred),) + ((("_icp", var.dpc_pred_icp),) if icp is not None else ()):
        a, b, n = emd_subsample(pred, gt, points)
        res = ops.emd_match(a, b, eps=eps)
        var["emd" + suffix] = res.emd
        var["emd_rounds" + suffix] = res.rounds
        var["emd_converged" + suffix] = res.converged
        var["emd_assignment" + suffix] = res.assignment
    var.emd_n = n


@torch.no_grad()
def iou_metrics(opt, var, res, close, icp=None):
    """`--eval.iou`: the volumetric IoU of the normalised prediction var.dpc_pred and the normalised ground truth var.dpc.points.  The
    ground truth is a bare point cloud, so BOTH solids are built the same way, in the one frame ops.voxel_frame gives the pair:
    splat to a shell of res^3 voxels, dilate `close` times so that pinholes close, fill what the exterior cannot reach, erode `close`
    times (ops.voxel_solid, csrc/voxel_solid.hip) -- a symmetric measure, like Chamfer, that charges for enclosed volume.  Sets
    var.iou [B] float64 (inter / union; 1 for an empty union, ops.mask_iou's convention; NaN where the frame is not finite),
    var.iou_inter / var.iou_union, var.iou_vox_pred / var.iou_vox_gt (the solids' voxels), var.iou_shell_pred / var.iou_shell_gt (the
    shells': a solid no larger than its shell did not fill) [B] int32, var.iou_bits_pred / var.iou_bits_gt [B,res,res] int64,
    var.iou_origin [B,3], var.iou_pitch [B] and var.iou_res (the int).  With `--eval.icp` (icp = icp_metrics' result): the same with
    the suffix _icp for var.dpc_pred_icp, in the frame of that cloud and the ground truth.  The raw metrics are untouched, nothing
    enters a loss."""
    gt = var.dpc.points.contiguous().float()
    for suffix, pred in (("", var.dpc_pred),) + ((("_icp", var.dpc_pred_icp),) if icp is not None else ()):
        pred = pred.contiguous().float()
        origin, pitch = ops.voxel_frame(pred, gt, res, close)
        solid_pred = ops.voxel_solid(pred, origin, pitch, res, close)
        solid_gt = ops.voxel_solid(gt, origin, pitch, res, close)
        inter, union = ops.voxel_iou(solid_pred.bits, solid_gt.bits)
        iou = torch.where(union > 0, inter.double() / union.clamp(min=1).double(), torch.ones_like(inter, dtype=torch.float64))
        finite = torch.isfinite(origin).all(dim=1) & torch.isfinite(pitch)
        var["iou" + suffix] = torch.where(finite, iou, torch.full_like(iou, float("nan")))
        var["iou_inter" + suffix], var["iou_union" + suffix] = inter, union
        var["iou_vox_pred" + suffix], var["iou_vox_gt" + suffix] = solid_pred.solid_voxels, solid_gt.solid_voxels
        var["iou_shell_pred" + suffix], var["iou_shell_gt" + suffix] = solid_pred.shell_voxels, solid_gt.shell_voxels
        var["iou_bits_pred" + suffix], var["iou_bits_gt" + suffix] = solid_pred.bits, solid_gt.bits
        var["iou_origin" + suffix], var["iou_pitch" + suffix] = origin, pitch
    var.iou_res = res


def voxel_centres(bits, origin, pitch):
    """bits [R,R] int64 (bit z of bits[x, y] is voxel (x, y, z)), origin [3], pitch scalar -> [n,3] fp32 on the host: the centres
    origin + (index + 0.5) pitch of the voxels that are set, in (x, y, z) order (the dump's {idx}_voxels_comp.ply)."""
    R = bits.shape[0]
    z = torch.arange(R, device=bits.device, dtype=torch.int64)
    index = ((bits.unsqueeze(-1) >> z) & 1).nonzero().float()
    return ((index + 0.5) * pitch.float() + origin.float()).cpu()


def _mesh_packed(var):
    """ops.isosurface_mesh(var.level_vox), built once and kept in var.mesh_packed.  var turns a tuple into a plain list, so the packed
    meshes it keeps (this one and var.mesh_dual_packed) are lists of the four fields and are read back as ops.PackedMesh(*list)."""
    if "mesh_packed" not in var:
        var.mesh_packed = list(ops.isosurface_mesh(var.level_vox))
    return ops.PackedMesh(*var.mesh_packed)


@torch.no_grad()
def mesh_stats(opt, var, sdf_network=None):
    """`--eval.mesh_stats`: is the mesh that is written a valid surface?  ops.mesh_topology (csrc/mesh_topology.hip) on the mesh of
    ops.isosurface_mesh(var.level_vox) -- the faces of {idx}_mesh.ply, _mesh_color.ply and _mesh_tex.obj -- with the vertices at the
    positions the level grid was sampled at, lo + v (hi - lo) / (S - 1), so that area and volume are in object units.  Sets
    var.mesh_stats: ops.MeshTopology as a dict (var keeps dicts with attribute access; a tuple would become a plain list) -- per image
    vertices, faces, edges, boundary / non-manifold / inconsistent edges, non-manifold vertices, degenerate faces, unreferenced
    vertices, components, largest_component_faces, euler, genus, the flags watertight, oriented, manifold, area, volume -- and
    face_component [F].  The packed mesh stays in var.mesh_packed (ops.PackedMesh's four fields, verts in grid-index units) and is taken
    from there when it is already present.  With `--eval.dual_mesh`: the same for the dual-contouring mesh in var.mesh_stats_dual,
    from var.mesh_dual_packed when --eval.mesh_dist left it there, else built here with sdf_network (var.mesh_dual then serves the
    dump); without a network and without that mesh the dual statistics are left out.  Nothing is repaired, nothing enters a loss."""
    lo, hi = opt.eval.range
    S = var.level_vox.shape[1]
    B = var.level_vox.shape[0]

    def measure(mesh):
        return ops.mesh_topology(*mesh._replace(verts=sampled_position(mesh.verts, lo, hi, S).contiguous()))._asdict()

    var.mesh_stats = measure(_mesh_packed(var))
    reg = options.dual_mesh_reg(opt)
    if reg is None:
        return
    if "mesh_dual_packed" not in var and sdf_network is not None:
        dual = meshes_dual(opt, sdf_network, var.proj_latent_sdf, var.level_vox, reg, keep=var)
        if "mesh_dual" not in var:
            var.mesh_dual = dual
        if "mesh_dual_packed" not in var:       # no crossing vertex in the whole batch
            var.mesh_dual_packed = list(ops.PackedMesh.empty(B, var.level_vox.device))
    if "mesh_dual_packed" in var:
        var.mesh_stats_dual = measure(ops.PackedMesh(*var.mesh_dual_packed))


@torch.no_grad()
def meshes_simplified(opt, var):
    """`--eval.simplify=k`: the mesh that is written, decimated.  ops.mesh_cluster_simplify (csrc/mesh_simplify.hip) on the packed mesh of
    ops.isosurface_mesh(var.level_vox) -- var.mesh_packed, built here as mesh_stats does when it is absent -- in grid-index units with
    origin 0, cells of k grid pitches and G = ceil((S - 1) / k) cells per axis (a ValueError naming eval.simplify when G > 128).
    Sets var.mesh_simplified, a dict (var keeps dicts with attribute access): the fields of ops.SimplifiedMesh (verts in grid-index units),
    cell = k, vertices_in, faces_in [B] and dist_mean, dist_max [B] float32 -- the distance from every ORIGINAL vertex to the simplified
    mesh (ops.point_mesh_distance), both at the positions the level grid was sampled at, lo + v (hi - lo) / (S - 1), in object units: the
    one-sided deviation paid for the smaller file; nan for an image whose simplified mesh has no face.  With `--eval.mesh_stats` also
    var.mesh_stats_simplified, ops.mesh_topology of the simplified mesh at those positions, as a dict.  Returns, and keeps in
    var.mesh_simplified_world for the dump, the per-image list of (vertices, faces) with meshes_device's v / S rescale, which overlays
    {idx}_mesh.ply.  Nothing is repaired, nothing enters a loss."""
    k, reg = options.simplify_settings(opt)
    lo, hi = opt.eval.range
    B, S = var.level_vox.shape[0], var.level_vox.shape[1]
    dev = var.level_vox.device
    G = -(-(S - 1) // k)
    if G > ops.MESH_SIMPLIFY_MAX_CELLS:
        raise ValueError("eval.simplify = %d gives %d cells per axis at a level grid of %d points; at most %d (choose eval.simplify >= %d)"
                         % (k, G, S, ops.MESH_SIMPLIFY_MAX_CELLS, -(-(S - 1) // ops.MESH_SIMPLIFY_MAX_CELLS)))
    mesh = _mesh_packed(var)
    res = ops.mesh_cluster_simplify(*mesh, (0.0, 0.0, 0.0), float(k), G, reg)
    to_object = lambda v: sampled_position(v, lo, hi, S).contiguous()
    v_in, f_out = mesh.v_count.tolist(), res.f_count.tolist()
    dist_mean = torch.full((B,), float("nan"), device=dev)
    dist_max = torch.full((B,), float("nan"), device=dev)
    if max(v_in, default=0) > 0 and res.faces.shape[0] > 0:
        _, rows = mesh.padded_rows()                                    # padding rows repeat the image's first vertex
        dist = ops.point_mesh_distance(to_object(mesh.verts)[rows].contiguous(), to_object(res.verts), res.faces.contiguous(),
                                       res.v_count, res.f_count, search="grid").dist2.sqrt()
        for b in range(B):
            if v_in[b] > 0 and f_out[b] > 0:
                dist_mean[b], dist_max[b] = dist[b, :v_in[b]].mean(), dist[b, :v_in[b]].max()
    var.mesh_simplified = dict(res._asdict(), cell=k, vertices_in=mesh.v_count.clone(), faces_in=mesh.f_count.clone(), dist_mean=dist_mean,
                               dist_max=dist_max)
    if options.mesh_stats_settings(opt):
        var.mesh_stats_simplified = ops.mesh_topology(*res.packed._replace(verts=to_object(res.verts)))._asdict()
    var.mesh_simplified_world = res.packed.split(written_position(res.verts, lo, hi, S))
    return var.mesh_simplified_world


@torch.no_grad()
def meshes_smoothed(opt, var):
    """`--mesh.smooth=n`: the mesh that is written, smoothed.  ops.mesh_smooth (csrc/mesh_smooth.hip) -- n Taubin iterations with
    mesh.smooth_lambda and the mu of mesh.smooth_band -- on the packed mesh of ops.isosurface_mesh(var.level_vox) -- var.mesh_packed,
    built here as mesh_stats does when it is absent -- in grid-index units, where every grid pitch is 1 on all three axes.
    Sets var.mesh_smoothed, a dict (var keeps dicts with attribute access): the fields of ops.SmoothedMesh (verts in grid-index units),
    iters, lam, mu, and area_before, area_after, volume_before, volume_after [B] float64 -- ops.mesh_topology's of the original and of
    the smoothed vertices at the positions the level grid was sampled at, lo + v (hi - lo) / (S - 1), in object units (the "before" pair
    is taken from var.mesh_stats when `--eval.mesh_stats` left it there); disp_* and rough_* are scaled to object units by (hi - lo) /
    (S - 1) on the host.  Returns, and keeps in var.mesh_smoothed_world for the dump, the per-image list of (vertices, faces) with
    meshes_device's v / S rescale, which overlays {idx}_mesh.ply.  The metrics keep sampling the unsmoothed surface; nothing enters a
    loss."""
    iters, lam, mu = options.smooth_settings(opt)
    lo, hi = opt.eval.range
    S = var.level_vox.shape[1]
    mesh = _mesh_packed(var)
    res = ops.mesh_smooth(*mesh, iters, lam, mu)
    to_object = lambda v: sampled_position(v, lo, hi, S).contiguous()
    after = ops.mesh_topology(*res.packed._replace(verts=to_object(res.verts)))
    before = var.mesh_stats if "mesh_stats" in var else ops.mesh_topology(*mesh._replace(verts=to_object(mesh.verts)))._asdict()
    pitch = (hi - lo) / (S - 1)
    scaled = {k: getattr(res, k) * pitch for k in ops.MESH_SMOOTH_MEASURES}
    var.mesh_smoothed = dict(res._asdict(), **scaled, iters=iters, lam=lam, mu=mu, area_before=before["area"], area_after=after.area,
                             volume_before=before["volume"], volume_after=after.volume)
    var.mesh_smoothed_world = res.packed.split(written_position(res.verts, lo, hi, S))
    return var.mesh_smoothed_world


def smoothed_lines(var):
    """One line per sample for {idx}_mesh_smooth.txt: idx iters lambda mu vertices free fixed_boundary isolated degree_max disp_mean
    disp_max rough_before rough_after area_before area_after volume_before volume_after (17 fields; one host read per field)."""
    r = var.mesh_smoothed
    ints = [torch.as_tensor(r[k]).cpu().tolist() for k in ("v_count",) + ops.MESH_SMOOTH_COUNTS]
    reals = [torch.as_tensor(r[k]).cpu().tolist() for k in ops.MESH_SMOOTH_MEASURES + ("area_before", "area_after", "volume_before",
                                                                                      "volume_after")]
    head = "%d %.17g %.17g" % (r["iters"], r["lam"], r["mu"])
    return ["%d %s %s %s" % (int(i), head, " ".join("%d" % col[b] for col in ints), " ".join("%.9g" % col[b] for col in reals))
            for b, i in enumerate(var.idx.cpu().tolist())]


SUBDIVIDE_MAX_STEP = 0.5    # the longest Newton step of meshes_subdivided, in grid pitches


def _ordered_sums(terms):
    """terms [..., n] float64, non-negative -> [...]: the sum over the last axis in a fixed order that depends on a term's position
    alone -- chunks of 16 consecutive terms added one at a time in ascending position, the chunk partials folded the same way, until one
    is left (15 elementwise additions a level, four levels for 65,536 terms).  Zeros appended to a row change no bit, so a row padded to
    another batch's width sums to the same bits."""
    x = terms
    while x.shape[-1] > 1:
        n = x.shape[-1]
        chunks = (n + 15) // 16
        x = torch.nn.functional.pad(x, (0, chunks * 16 - n)).view(*x.shape[:-1], chunks, 16)
        acc = x[..., 0]
        for t in range(1, 16):
            acc = acc + x[..., t]
        x = acc
    return x[..., 0] if x.shape[-1] else x.sum(-1)


def _sdf_at(sdf_network, proj_latent_sdf):
    """-> ask(query, B, P, want_grad): query [B P, 3] in the padded one-launch layout (P a multiple of 16 rows per image) -> (sdf [B P]
    fp32, d sdf / d position [B P, 3] fp32 or None), by one ops.sdf_forward on weight images packed once here; architectures outside the
    compiled family (sdf_network.eager) run the same step on stock operators (model/eager_path.py)."""
    if getattr(sdf_network, "eager", False):
        from ..model import eager_path

        def ask(query, B, P, want_grad):
            sdf, _, grad = eager_path.sdf_conditional_output(sdf_network, B, query, proj_latent_sdf, compute_grad=want_grad)
            return sdf.detach().reshape(-1).float(), grad.detach().float().contiguous() if want_grad else None
        return ask
    w_pack, cbias = sdf_network.packed(proj_latent_sdf)

    def ask(query, B, P, want_grad):
        sdf, grad, _ = ops.sdf_forward(query, w_pack, cbias, P, symmetric=bool(sdf_network.force_symmetry), want_grad=want_grad, want_feat=False)
        return sdf.reshape(-1).float(), grad.float() if want_grad else None
    return ask


@torch.no_grad()
def meshes_subdivided(opt, var, sdf_network):
    """`--mesh.subdivide=n`: the mesh that is written, refined and put back on the network's zero set.  ops.mesh_subdivide
    (csrc/mesh_subdivide.hip) -- n levels of Loop subdivision -- on the packed mesh of ops.isosurface_mesh(var.level_vox) --
    var.mesh_packed, built here as mesh_stats does when it is absent -- in grid-index units, where every grid pitch is 1 on all three
    axes.  Then k = mesh.subdivide_project rounds of: one SDF evaluation with gradient at sampled_position(v), in mesh_attributes' padded
    one-launch layout (sdf_network.eager: stock operators), and one ops.mesh_project_step with scale = (S - 1) / (hi - lo), which turns
    the Newton step from object units into grid pitches, and max_step = 0.5 pitches; fixed vertices (the open rim and its midpoints,
    non-manifold edges) keep their bits.  After the last round one value-only evaluation.  k = 0 asks the network nothing.
    Sets var.mesh_subdivided, a dict (var keeps dicts with attribute access): the fields of ops.SubdividedMesh (verts in grid-index
    units, after the projection), levels, project, vertices_in, faces_in [B] int64 and, [B] float64 on the device: resid_before /
    resid_after, the mean |sdf| over the vertices that are not fixed before the first step and after the last (nan for k = 0; 0 for
    an image without such a vertex); disp_mean / disp_max, how far the projection moved them, in object units; area_before, area_after,
    volume_before, volume_after, ops.mesh_topology's of the original and of the refined mesh at the positions the level grid was
    sampled at, in object units (the "before" pair is taken from var.mesh_stats when `--eval.mesh_stats` left it there).  The means
    are float64 sums in a fixed order (_ordered_sums): the same bits whatever batch the sample is in.  Returns, and keeps in
    var.mesh_subdivided_world for the dump, the per-image list of (vertices, faces) with meshes_device's v / S rescale, which overlays
    {idx}_mesh.ply.  The metrics keep sampling the marching-cubes surface; nothing enters a loss."""
    levels, project = options.subdivide_settings(opt)
    lo, hi = opt.eval.range
    S = var.level_vox.shape[1]
    mesh = _mesh_packed(var)
    B = mesh.v_count.shape[0]
    res = ops.mesh_subdivide(*mesh, levels)
    sub = res.packed
    dev = sub.verts.device
    pitch = (hi - lo) / (S - 1)
    start = verts = sub.verts
    nan = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    measures = dict(resid_before=nan, resid_after=nan, disp_mean=torch.zeros_like(nan), disp_max=torch.zeros_like(nan))
    P, rows = sub.padded_rows(16)
    if project > 0 and P > 0:
        ask = _sdf_at(sdf_network, var.proj_latent_sdf)
        real = torch.arange(P, device=dev)[None] < sub.v_count.to(dev)[:, None]         # [B, P]: the rows that are a vertex, in packed order
        flat, real_flat = rows.reshape(-1), real.reshape(-1)
        query = lambda v: sampled_position(v[flat], lo, hi, S).contiguous()
        first = None
        for _ in range(project):
            sdf, grad = ask(query(verts), B, P, True)
            first = sdf if first is None else first
            verts = ops.mesh_project_step(verts, sdf[real_flat].contiguous(), grad[real_flat].contiguous(), res.fixed, 1.0 / pitch,
                                          SUBDIVIDE_MAX_STEP)
        last, _ = ask(query(verts), B, P, False)
        free = real & ~res.fixed[flat].view(B, P)
        d = verts.double() - start.double()
        moved = (torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) * pitch)[flat].view(B, P)
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        terms = torch.stack([torch.where(free, t, zero) for t in (first.view(B, P).double().abs(), last.view(B, P).double().abs(), moved)])
        n_free = free.sum(1)
        mean = torch.where(n_free > 0, _ordered_sums(terms) / n_free.double().clamp_min(1.0), zero)
        measures = dict(resid_before=mean[0], resid_after=mean[1], disp_mean=mean[2], disp_max=terms[2].amax(1))
    elif project > 0:
        measures.update(resid_before=torch.zeros_like(nan), resid_after=torch.zeros_like(nan))
    to_object = lambda v: sampled_position(v, lo, hi, S).contiguous()
    after = ops.mesh_topology(*sub._replace(verts=to_object(verts)))
    before = var.mesh_stats if "mesh_stats" in var else ops.mesh_topology(*mesh._replace(verts=to_object(mesh.verts)))._asdict()
    var.mesh_subdivided = dict(res._replace(verts=verts)._asdict(), **measures, levels=levels, project=project,
                               vertices_in=mesh.v_count.long(), faces_in=mesh.f_count.long(), area_before=before["area"],
                               area_after=after.area, volume_before=before["volume"], volume_after=after.volume)
    var.mesh_subdivided_world = sub.split(written_position(verts, lo, hi, S))
    return var.mesh_subdivided_world


def subdivided_lines(var):
    """One line per sample for {idx}_mesh_subdiv.txt: idx levels project vertices_in vertices_out faces_in faces_out edges sharp_edges
    fixed resid_before resid_after disp_mean disp_max area_before area_after volume_before volume_after (18 fields; one host read per
    field)."""
    r = var.mesh_subdivided
    ints = [torch.as_tensor(r[k]).cpu().tolist() for k in ("vertices_in", "v_count", "faces_in", "f_count", "edges", "sharp_edges",
                                                           "fixed_vertices")]
    reals = [torch.as_tensor(r[k]).cpu().tolist() for k in ("resid_before", "resid_after", "disp_mean", "disp_max", "area_before",
                                                            "area_after", "volume_before", "volume_after")]
    return ["%d %d %d %s %s" % (int(i), r["levels"], r["project"], " ".join("%d" % col[b] for col in ints),
                                " ".join("%.9g" % col[b] for col in reals)) for b, i in enumerate(var.idx.cpu().tolist())]


@torch.no_grad()
def meshes_decimated(opt, var):
    """`--mesh.decimate=F`: the mesh that is written, brought to a face budget.  ops.mesh_decimate (csrc/mesh_decimate.hip) -- quadric edge
    collapses down to mesh.decimate faces per sample, with mesh.decimate_reg and at most mesh.decimate_rounds rounds -- on the packed mesh
    of ops.isosurface_mesh(var.level_vox) -- var.mesh_packed, built here as mesh_stats does when it is absent -- in grid-index units.
    Sets var.mesh_decimated, a dict (var keeps dicts with attribute access): the fields of ops.DecimatedMesh (verts in grid-index units),
    target, vertices_in, faces_in [B] int64, dist_mean, dist_max [B] float32 -- the distance from every ORIGINAL vertex to the decimated
    mesh (ops.point_mesh_distance), in object units as in meshes_simplified; nan for an image whose decimated mesh has no face -- and
    area_before, area_after, volume_before, volume_after [B] float64, ops.mesh_topology's of the original and of the decimated mesh at
    the positions the level grid was sampled at, in object units (the "before" pair is taken from var.mesh_stats when `--eval.mesh_stats`
    left it there).  Returns, and keeps in var.mesh_decimated_world for the dump, the per-image list of (vertices, faces) with
    meshes_device's v / S rescale, which overlays {idx}_mesh.ply.  The metrics keep sampling the marching-cubes surface; nothing enters a
    loss."""
    target, reg, rounds = options.decimate_settings(opt)
    lo, hi = opt.eval.range
    B, S = var.level_vox.shape[0], var.level_vox.shape[1]
    dev = var.level_vox.device
    mesh = _mesh_packed(var)
    res = ops.mesh_decimate(*mesh, target, reg, rounds)
    to_object = lambda v: sampled_position(v, lo, hi, S).contiguous()
    v_in, f_out = mesh.v_count.tolist(), res.f_count.tolist()
    dist_mean = torch.full((B,), float("nan"), device=dev)
    dist_max = torch.full((B,), float("nan"), device=dev)
    if max(v_in, default=0) > 0 and res.faces.shape[0] > 0:
        _, rows = mesh.padded_rows()                                    # padding rows repeat the image's first vertex
        dist = ops.point_mesh_distance(to_object(mesh.verts)[rows].contiguous(), to_object(res.verts), res.faces.contiguous(),
                                       res.v_count, res.f_count, search="grid").dist2.sqrt()
        for b in range(B):
            if v_in[b] > 0 and f_out[b] > 0:
                dist_mean[b], dist_max[b] = dist[b, :v_in[b]].mean(), dist[b, :v_in[b]].max()
    after = ops.mesh_topology(*res.packed._replace(verts=to_object(res.verts)))
    before = var.mesh_stats if "mesh_stats" in var else ops.mesh_topology(*mesh._replace(verts=to_object(mesh.verts)))._asdict()
    var.mesh_decimated = dict(res._asdict(), target=target, vertices_in=mesh.v_count.long().clone(), faces_in=mesh.f_count.long().clone(),
                              dist_mean=dist_mean, dist_max=dist_max, area_before=before["area"], area_after=after.area,
                              volume_before=before["volume"], volume_after=after.volume)
    var.mesh_decimated_world = res.packed.split(written_position(res.verts, lo, hi, S))
    return var.mesh_decimated_world


def decimated_lines(var):
    """One line per sample for {idx}_mesh_decimated.txt: idx target vertices_in vertices_out faces_in faces_out rounds collapses
    rejected_link rejected_flip fixed reached dist_mean dist_max area_before area_after volume_before volume_after (18 fields; one host
    read per field)."""
    r = var.mesh_decimated
    ints = [torch.as_tensor(r[k]).cpu().tolist() for k in ("vertices_in", "v_count", "faces_in", "f_count", "rounds", "collapses",
                                                           "rejected_link", "rejected_flip", "fixed_vertices", "reached")]
    reals = [torch.as_tensor(r[k]).cpu().tolist() for k in ("dist_mean", "dist_max", "area_before", "area_after", "volume_before",
                                                            "volume_after")]
    return ["%d %d %s %s" % (int(i), r["target"], " ".join("%d" % col[b] for col in ints), " ".join("%.9g" % col[b] for col in reals))
            for b, i in enumerate(var.idx.cpu().tolist())]


AO_STEP = 0.5      # grid pitches between the samples of a ray of mesh_ambient_occlusion: half a cell, so no cell on the way is jumped
AO_BIAS = 1.0      # the rays start one normal length (a grid pitch: the normals are unit) off the surface, clear of the vertex's own cells


def _grey_bytes(ao):
    """ao [...] fp32 -> uint8: trunc(clamp(ao, 0, 1) * 255), the recipe of the PNG dumps and of mesh_attributes."""
    return (ao.clamp(0, 1) * 255).to(torch.uint8)


@torch.no_grad()
def mesh_ambient_occlusion(opt, var, sdf_network):
    """`--mesh.ao`: where is the written mesh concave?  ops.level_ambient_occlusion (csrc/level_ao.hip) at every vertex of the packed
    mesh of ops.isosurface_mesh(var.level_vox) -- var.mesh_packed, built here as mesh_stats does when it is absent; its verts are in
    grid-index units already -- against var.level_vox itself (so --hip.largest_component applies), with the unit SDF gradient at
    sampled_position(v) as the normal: one SDF evaluation with gradient in mesh_attributes' padded one-launch layout
    (sdf_network.eager: stock operators).  Reach mesh.ao_radius (S - 1) pitches, samples AO_STEP apart, start AO_BIAS off the surface.
    Sets var.mesh_ao, a dict (var keeps dicts with attribute access): ao [V] fp32, mask [V] int64, normals [V,3] fp32, v_count, radius
    and step (grid pitches), and per image, [B] float64 on the device: ao_mean (a float64 sum in a fixed order, _ordered_sums), ao_min,
    ao_max, open_share (the share of vertices whose 64 rays are all open); nan for an image without a vertex.  Returns, and keeps in
    var.mesh_ao_world for the dump, per image (vertices, faces, normals, grey): {idx}_mesh.ply's vertices and faces (meshes_device's
    v / S rescale) and trunc(clamp(ao, 0, 1) * 255) in all three colour channels.  Nothing is measured against the ground truth and
    nothing enters a loss."""
    lo, hi = opt.eval.range
    level = var.level_vox.float().contiguous()
    B, S = level.shape[0], level.shape[1]
    radius = options.ao_settings(opt, S)
    dev = level.device
    mesh = _mesh_packed(var)
    v_count = mesh.v_count.to(dev)
    P, rows = mesh.padded_rows(16)
    nan = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    stats = dict(ao_mean=nan, ao_min=nan, ao_max=nan, open_share=nan)
    if P == 0:
        ao, mask = torch.zeros(0, device=dev), torch.zeros(0, dtype=torch.int64, device=dev)
        normals = torch.zeros(0, 3, device=dev)
    else:
        real = torch.arange(P, device=dev)[None] < v_count[:, None]                      # [B, P]: the rows that are a vertex, in packed order
        flat = rows.reshape(-1)
        _, grad = _sdf_at(sdf_network, var.proj_latent_sdf)(sampled_position(mesh.verts[flat], lo, hi, S).contiguous(), B, P, True)
        normals = torch.nn.functional.normalize(grad[real.reshape(-1)], dim=1, eps=1e-12).contiguous()
        image = torch.repeat_interleave(torch.arange(B, device=dev, dtype=torch.int32), v_count)
        ao, mask = ops.level_ambient_occlusion(level, mesh.verts.contiguous(), normals, image, radius, step=AO_STEP, bias=AO_BIAS)
        padded = ao.double()[flat].view(B, P)
        zero, inf = torch.zeros((), dtype=torch.float64, device=dev), torch.full((), float("inf"), dtype=torch.float64, device=dev)
        n = v_count.double()
        some = v_count > 0
        share = lambda x: torch.where(some, x / n.clamp_min(1.0), nan)
        stats = dict(ao_mean=share(_ordered_sums(torch.where(real, padded, zero))),
                     ao_min=torch.where(some, torch.where(real, padded, inf).amin(1), nan),
                     ao_max=torch.where(some, torch.where(real, padded, -inf).amax(1), nan),
                     open_share=share((real & (mask[flat].view(B, P) == -1)).sum(1).double()))
    var.mesh_ao = dict(ao=ao, mask=mask, normals=normals, v_count=mesh.v_count, radius=radius, step=AO_STEP, **stats)
    grey = _grey_bytes(ao)[:, None].expand(-1, 3)
    written = mesh.split(written_position(mesh.verts, lo, hi, S))       # meshes_device's expression: the same bytes as {idx}_mesh.ply
    var.mesh_ao_world = [(*written[b], n_b, g_b) for b, ((n_b, _), (g_b, _)) in enumerate(zip(mesh.split(normals), mesh.split(grey)))]
    return var.mesh_ao_world


def ao_lines(var):
    """One line per sample for {idx}_mesh_ao.txt: idx vertices radius step ao_mean ao_min ao_max open_share (8 fields; radius and step in
    grid pitches; one host read per field)."""
    r = var.mesh_ao
    verts = torch.as_tensor(r["v_count"]).cpu().tolist()
    reals = [torch.as_tensor(r[k]).cpu().tolist() for k in ("ao_mean", "ao_min", "ao_max", "open_share")]
    return ["%d %d %.9g %.9g %s" % (int(i), verts[b], r["radius"], r["step"], " ".join("%.9g" % col[b] for col in reals))
            for b, i in enumerate(var.idx.cpu().tolist())]


@torch.no_grad()
def mesh_ao_atlas(opt, var, textured):
    """`--mesh.ao` with `--eval.texture`: per image the AO atlas uint8 [A,A] in the layout of the colour atlas of `textured`
    (mesh_texture of var.level_vox).  ops.texture_queries yields the texels' positions again; those of the texels that hold a face go
    back to grid-index units by (p - lo) * ((S - 1) / (hi - lo)), their normals are decoded from the normal atlas as 2 x / 255 - 1, and
    one ops.level_ambient_occlusion call with mesh_ambient_occlusion's reach, step and bias serves the batch.  A used texel holds
    trunc(clamp(ao, 0, 1) * 255), every other one 127.  The TexturedMesh list is not changed."""
    lo, hi = opt.eval.range
    T = options.texture_texels(opt, always=True)
    level = var.level_vox.float().contiguous()
    B, S = level.shape[0], level.shape[1]
    dev = level.device
    mesh = _mesh_packed(var)
    v_start, f_start, F = mesh.starts()
    A, _, rows = ops.texture_layout(max(F, default=0), T)
    blank = torch.full((64, 64), 127, dtype=torch.uint8, device=dev)
    if rows == 0:
        return [blank] * B
    assert all(m.faces.shape[0] == F[b] and (F[b] == 0 or m.atlas.shape[0] == A) for b, m in enumerate(textured)), \
        "the texture was baked for another mesh"
    query, face_of_texel = ops.texture_queries(mesh.verts, mesh.faces, v_start, f_start, F, A, T, lo, hi, S, rows)
    used = (face_of_texel.reshape(-1) >= 0).nonzero().reshape(-1)                      # texel b rows A + y A + x, ascending
    grey127 = torch.full((rows, A, 3), 127, dtype=torch.uint8, device=dev)
    bytes_n = torch.stack([m.normal_atlas[:rows] if F[b] else grey127 for b, m in enumerate(textured)]).reshape(-1, 3)
    points = ((query[used] - lo) * ((S - 1) / (hi - lo))).contiguous()
    normals = (2 * bytes_n[used].float() / 255 - 1).contiguous()
    image = (used // (rows * A)).int()
    ao = ops.level_ambient_occlusion(level, points, normals, image, options.ao_settings(opt, S), step=AO_STEP, bias=AO_BIAS).ao
    atlas = torch.full((B, A, A), 127, dtype=torch.uint8, device=dev)
    top = torch.full((B * rows * A,), 127, dtype=torch.uint8, device=dev)
    top[used] = _grey_bytes(ao)
    atlas[:, :rows] = top.view(B, rows, A)
    return [atlas[b] if F[b] else blank for b in range(B)]


@torch.no_grad()
def mesh_shade(opt, var, render, pose):
    """`--mesh.ao` with `--eval.mesh_render`: a MeshRender of the mesh of var.level_vox (mesh_render) from `pose` [B,3,4] or [B,V,3,4],
    lit -> (shaded, clay), both [B,V,H,W,3] in [0, 1].  Per pixel ao is the barycentric mix (b0 a0 + b1 a1) + b2 a2 of the winning
    face's three vertex values of var.mesh_ao (render.face, render.bary); lambert = |n . z_cam| / |n| with n = 2 render.normal - 1 and
    z_cam the third row of the pose's rotation -- a two-sided head light; shade = ao (0.3 + 0.7 lambert); shaded = render.rgb shade and
    clay = 0.8 shade in all three channels; a miss is data.bgcolor in both.  The MeshRender is not changed."""
    mesh = _mesh_packed(var)
    dev = render.face.device
    B, V, H, W = render.face.shape
    bg = torch.full((), float(opt.data.bgcolor), device=dev)
    covered = (render.face >= 0).view(B, V, H, W, 1)
    if mesh.faces.shape[0] == 0:
        miss = bg.expand(B, V, H, W, 3).contiguous()
        return miss, miss.clone()
    v_start, f_start, _ = mesh.starts()
    first_f = torch.tensor(f_start, device=dev).view(B, 1, 1, 1)
    first_v = torch.tensor(v_start, device=dev).view(B, 1, 1, 1, 1)
    face = (render.face.clamp(min=0).long() + first_f).clamp(max=mesh.faces.shape[0] - 1)     # a miss reads some face, unused
    corner = (mesh.faces[face.view(-1)].long().view(B, V, H, W, 3) + first_v).clamp(max=mesh.verts.shape[0] - 1)
    a = var.mesh_ao["ao"][corner.view(-1)].view(B, V, H, W, 3)
    t = render.bary * a
    ao = (t[..., 0] + t[..., 1]) + t[..., 2]
    pose = pose.float().to(dev)
    z_cam = (pose[:, None] if pose.dim() == 3 else pose)[..., 2, :3].reshape(B, -1, 1, 1, 3)
    n = 2 * render.normal - 1
    lambert = (n * z_cam).sum(-1).abs() / n.norm(dim=-1).clamp_min(1e-12)
    shade = (ao * (0.3 + 0.7 * lambert)).unsqueeze(-1)
    shaded = torch.where(covered, render.rgb * shade, bg)
    clay = torch.where(covered, (0.8 * shade).expand(-1, -1, -1, -1, 3), bg)
    return shaded, clay


# the order of {idx}_mesh_selfx.txt's lines; "decimated" is there with `--mesh.decimate` only
INTERSECT_VARIANTS = ("mc", "dual", "simplified", "smooth", "subdiv", "decimated")
_INTERSECT_HELD = {"simplified": "mesh_simplified", "smooth": "mesh_smoothed", "subdiv": "mesh_subdivided", "decimated": "mesh_decimated"}


@torch.no_grad()
def mesh_intersections(opt, var, sdf_network=None):
    """`--mesh.self_intersect`: does a written mesh pass through itself?  ops.mesh_self_intersections (csrc/mesh_intersect.hip) on every
    mesh variant this run writes, in the order of INTERSECT_VARIANTS: "mc", the marching-cubes mesh (var.mesh_packed, built here as
    mesh_stats does when it is absent); "dual" with `--eval.dual_mesh` (var.mesh_dual_packed, built here with sdf_network when no earlier
    step left it there; without a network and without that mesh the variant is left out); "simplified", "smooth", "subdiv" and "decimated"
    with `--eval.simplify`, `--mesh.smooth`, `--mesh.subdivide` and `--mesh.decimate`, the meshes eval_metrics' meshers left in var.  Each is tested as it is held:
    packed, in grid-index units.  The rule is strict (proper crossings only; see the op), so every counted pair truly intersects and the
    count is a lower bound.  Sets var.mesh_intersections, a dict per variant (var keeps dicts with attribute access) of the fields of
    ops.MeshIntersections and v_count, f_count [B] int64 on the host.  Runs after the meshers; nothing is repaired, nothing enters a loss."""
    B = var.level_vox.shape[0]
    found = {"mc": _mesh_packed(var)}
    reg = options.dual_mesh_reg(opt)
    if reg is not None:
        if "mesh_dual_packed" not in var and sdf_network is not None:
            dual = meshes_dual(opt, sdf_network, var.proj_latent_sdf, var.level_vox, reg, keep=var)
            if "mesh_dual" not in var:
                var.mesh_dual = dual                # serves the dump
            if "mesh_dual_packed" not in var:       # no crossing vertex in the whole batch
                var.mesh_dual_packed = list(ops.PackedMesh.empty(B, var.level_vox.device))
        if "mesh_dual_packed" in var:
            found["dual"] = ops.PackedMesh(*var.mesh_dual_packed)
    for variant, key in _INTERSECT_HELD.items():
        if key in var:
            found[variant] = ops.PackedMesh(*(var[key][k] for k in ("verts", "faces", "v_count", "f_count")))
    out = {}
    for variant in INTERSECT_VARIANTS:
        if variant in found:
            mesh = found[variant]
            res = ops.mesh_self_intersections(mesh.verts.contiguous(), mesh.faces.contiguous(), mesh.v_count, mesh.f_count)
            out[variant] = dict(res._asdict(), v_count=mesh.v_count.long().cpu(), f_count=mesh.f_count.long().cpu())
    var.mesh_intersections = out
    return out


def _intersection_meshes(var, variant):
    """The packed mesh (grid-index units) a variant of var.mesh_intersections was measured on."""
    if variant == "mc":
        return _mesh_packed(var)
    if variant == "dual":
        return ops.PackedMesh(*var.mesh_dual_packed)
    held = var[_INTERSECT_HELD[variant]]
    return ops.PackedMesh(*(held[k] for k in ("verts", "faces", "v_count", "f_count")))


def intersection_lines(var):
    """Per sample the text of {idx}_mesh_selfx.txt: one line per variant of var.mesh_intersections, in INTERSECT_VARIANTS' order --
    idx variant faces degenerate box_pairs pairs pairs_vertex faces_hit first_face first_partner (10 fields): first_face is the lowest
    face of the variant's mesh that crosses another, first_partner the lowest face it crosses; both -1 without a hit.  The lines of a
    sample are joined by newlines (util_vis.dump_lines writes one text per sample); one host read per field."""
    idx = var.idx.cpu().tolist()
    text = [[] for _ in idx]
    for variant in INTERSECT_VARIANTS:
        r = var.mesh_intersections.get(variant)
        if r is None:
            continue
        cols = [torch.as_tensor(r[k]).cpu().tolist() for k in ("f_count", "degenerate", "box_pairs", "pairs", "pairs_vertex", "faces_hit")]
        hits, partner = r["hits"].cpu(), r["partner"].cpu()
        start = 0
        for b, i in enumerate(idx):
            nf = cols[0][b]
            hit = (hits[start:start + nf] > 0).nonzero()
            first = int(hit[0]) if len(hit) else -1
            other = int(partner[start + first]) if first >= 0 else -1
            text[b].append("%d %s %s %d %d" % (int(i), variant, " ".join("%d" % c[b] for c in cols), first, other))
            start += nf
    return ["\n".join(lines) for lines in text]


def intersection_hit_meshes(opt, var, variant):
    """-> (rows, meshes): the samples (positions in the batch) whose `variant` mesh has a face in a hit pair and, for each, (vertices,
    faces) of the HIT faces alone -- their vertices renumbered in ascending order -- with meshes_device's v / S rescale, which overlays
    {idx}_mesh.ply: what {idx}_mesh_selfx_{variant}.ply holds."""
    lo, hi = opt.eval.range
    S = var.level_vox.shape[1]
    r = var.mesh_intersections[variant]
    mesh = _intersection_meshes(var, variant)
    world = mesh.split(written_position(mesh.verts, lo, hi, S))
    f_off = mesh.offsets()[1].tolist()
    faces_hit = torch.as_tensor(r["faces_hit"]).cpu().tolist()
    rows, meshes = [], []
    for b, (v, f) in enumerate(world):
        if faces_hit[b] > 0:
            keep = f[r["hits"][f_off[b]:f_off[b + 1]] > 0].long()
            used, renumbered = torch.unique(keep, return_inverse=True)
            rows.append(b)
            meshes.append((v[used].contiguous(), renumbered.int().contiguous()))
    return rows, meshes


_FLIP_PRED = [[1, 0, 0], [0, -1, 0], [0, 0, -1]]
_FLIP_GT = [[-1, 0, 0], [0, 1, 0], [0, 0, 1]]


@torch.no_grad()
def eval_metrics(opt, var, sdf_network, vis_only=False):
    # every optional metric's setting, read once: None (or False) while its switch is off, else the arguments of its function
    icp, normals_k, emd, iou = (f(opt) for f in (options.icp_settings, options.normal_settings, options.emd_settings, options.iou_settings))
    mesh_dist = None if vis_only else options.mesh_dist_settings(opt)
    want_stats, simplify = options.mesh_stats_settings(opt), options.simplify_settings(opt)
    smooth, subdivide = options.smooth_settings(opt), options.subdivide_settings(opt)
    decimate = options.decimate_settings(opt)
    self_intersect = options.self_intersect_settings(opt)
    shade = options.ao_settings(opt)
    points_3D = get_dense_3D_grid(opt, var)
    B = points_3D.shape[0]
    level_vox = compute_level_grid(opt, sdf_network, var.proj_latent_sdf, points_3D)
    if largest_component_enabled(opt):      # detached floaters leave the solid before anything is meshed, sampled or dumped from it
        level_vox, stats = ops.level_largest_component(level_vox.contiguous(), 0.0)
        var.component_stats = stats._asdict()               # (var keeps a dict with attribute access; a tuple would become a plain list)
    var.eval_vox = points_3D.view(B, -1, 3)
    var.level_vox = level_vox                                           # kept for the mesh dump (meshes_device), not recomputed there
    dev = var.idx.device
    if HAVE_MESHING:
        *level_grids, = level_vox.cpu().numpy()
        meshes, pointclouds = convert_to_explicit(opt, level_grids, isoval=0., to_pointcloud=True)
        var.mesh_pred = meshes
        var.dpc_pred = torch.tensor(pointclouds, dtype=torch.float32, device=dev)
    else:   # stay on the device: marching-cubes triangles + area-uniform samples (csrc/isosurface.hip)
        lo, hi = opt.eval.range
        var.dpc_pred, var.mesh_pred = surface_points_device(level_vox, lo, hi, opt.eval.num_points,
                                                            seed=int(var.idx[0]) if len(var.idx) else 0)
    points_object = var.dpc_pred                                        # the samples in the object frame (normal_metrics)
    if opt.data.dataset in ["openimage"]:
        var.f_score = torch.zeros(B, len(opt.eval.f_thresholds)).to(dev)
        var.cd_acc = torch.zeros(B).to(dev); var.cd_comp = torch.zeros(B).to(dev)
        return None if vis_only else (torch.tensor(0).to(dev), torch.tensor(0).to(dev))
    rot = lambda Rm, P: (Rm @ P.permute(0, 2, 1)).permute(0, 2, 1).contiguous()
    var.dpc_pred = rot(var.pose[..., :3], var.dpc_pred)
    var.dpc.points = rot(var.pose_gt[..., :3], var.dpc.points)
    if opt.data.dataset in ["pix3d"]:
        fp = torch.tensor(_FLIP_PRED).float().to(dev).unsqueeze(0).expand(B, 3, 3)
        fg = torch.tensor(_FLIP_GT).float().to(dev).unsqueeze(0).expand(B, 3, 3)
        var.dpc_pred = rot(fp, var.dpc_pred)
        var.dpc.points = rot(fg, var.dpc.points)
    frame = normalize_pc_params(var.dpc_pred) if mesh_dist is not None else None      # the samples' centre and scale (mesh_metrics)
    var.dpc_pred = normalize_pc(var.dpc_pred)
    var.dpc.points = normalize_pc(var.dpc.points)
    if vis_only:
        if want_stats:                          # vis_{ep}/mesh_stats.txt of --hip.train_vis
            mesh_stats(opt, var, sdf_network)
        if simplify is not None:                # vis_{ep}/{idx}_mesh_simplified.ply
            meshes_simplified(opt, var)
        if smooth is not None:                  # vis_{ep}/{idx}_mesh_smooth.ply and .txt
            meshes_smoothed(opt, var)
        if subdivide is not None:               # vis_{ep}/{idx}_mesh_subdiv.ply and .txt
            meshes_subdivided(opt, var, sdf_network)
        if decimate is not None:                # vis_{ep}/{idx}_mesh_decimated.ply and .txt
            meshes_decimated(opt, var)
        if self_intersect:                      # vis_{ep}/{idx}_mesh_selfx.txt: after the meshers, on what they left in var
            mesh_intersections(opt, var, sdf_network)
        if shade is not None:                   # vis_{ep}/{idx}_mesh_ao.ply and .txt
            mesh_ambient_occlusion(opt, var, sdf_network)
        return
    dist_acc, dist_comp, idx1, idx2 = chamfer_distance(opt, X1=var.dpc_pred, X2=var.dpc.points)
    var.f_score = compute_fscore(dist_acc, dist_comp, opt.eval.f_thresholds)
    assert dist_acc.shape[1] == opt.eval.num_points
    var.cd_acc = dist_acc.mean(dim=1)
    var.cd_comp = dist_comp.mean(dim=1)
    aligned = None
    if icp is not None:                     # beside the raw metrics, never in their place
        aligned = icp_metrics(opt, var, *icp)
    if normals_k is not None:               # likewise
        normal_metrics(opt, var, sdf_network, points_object, idx1, idx2, normals_k, icp=aligned)
    if mesh_dist is not None:               # likewise
        var.dist_acc, var.dist_comp = dist_acc, dist_comp
        mesh_metrics(opt, var, sdf_network, frame)
    if emd is not None:                     # likewise
        emd_metrics(opt, var, *emd, icp=aligned)
    if iou is not None:                     # likewise
        iou_metrics(opt, var, *iou, icp=aligned)
    if want_stats:                          # likewise
        mesh_stats(opt, var, sdf_network)
    if simplify is not None:                # likewise
        meshes_simplified(opt, var)
    if smooth is not None:                  # post-processing of the written mesh: no metric reads it
        meshes_smoothed(opt, var)
    if subdivide is not None:               # likewise
        meshes_subdivided(opt, var, sdf_network)
    if decimate is not None:                # likewise
        meshes_decimated(opt, var)
    if self_intersect:                      # a check of what is written, after the meshers: no metric reads it
        mesh_intersections(opt, var, sdf_network)
    if shade is not None:                   # shading of what is written: no metric reads it
        mesh_ambient_occlusion(opt, var, sdf_network)
    return dist_acc.mean(), dist_comp.mean()
