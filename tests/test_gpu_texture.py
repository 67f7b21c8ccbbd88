"""Textured OBJ meshes from a per-triangle atlas bake: csrc/texture_bake.hip (ops.texture_queries / texture_pack / texture_sample),
eval_3D.mesh_texture and `--eval.texture`.

What is pinned: the three kernels bit for bit against tests/texture_ref.py (the numpy restatement of include/shapeclipper_hip.h); the
round trip layout -> texture coordinates -> bilinear look-up against float64 within a counted rounding budget; the packed colours
bit-level against the existing chain (rgb_points_forward) and within tests/test_gpu_mesh_attributes.py's float64 budget of the oracle;
that slabbing and batching change no byte; the eager path; Runner.evaluate / evaluate_sharded writing the four files per sample and
texture.txt without changing any other output."""
import os

import numpy as np
import pytest
import torch

import texture_ref as ref
from test_gpu_mesh_attributes import _check_quantised, _opt, _reference, _sphere_level

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LO, HI = -0.6, 0.6                      # eval.range of the shipped options: neither bound is an fp32 number
TEXELS = (4, 5, 8)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_MESHES = {}


def _mesh(kinds, S=16):
    """The indexed marching-cubes mesh of a batch of analytic grids ("a": sphere r = 0.3, "b": sphere r = 0.41, "e": empty, "2": two
    spheres), computed once per batch: (verts, faces on the device, v_start, f_start, f_count lists, numpy per-image (verts, faces))."""
    from shapeclipper_amd import ops
    key = (kinds, S)
    if key not in _MESHES:
        grid = dict(a=lambda: ref.sphere_level(S, 0.3), b=lambda: ref.sphere_level(S, 0.41, (0.02, -0.03, 0.01)),
                    e=lambda: ref.empty_level(S), **{"2": lambda: ref.two_sphere_level(S)})
        level = _dev(np.stack([grid[k]() for k in kinds]))
        verts, faces, vc, fc = ops.isosurface_mesh(level)
        v_end, f_end = np.cumsum(vc.numpy()).tolist(), np.cumsum(fc.numpy()).tolist()
        v_start, f_start = [0] + v_end[:-1], [0] + f_end[:-1]
        vn, fn = verts.cpu().numpy(), faces.cpu().numpy()
        per = [(vn[v_start[b]:v_end[b]], fn[f_start[b]:f_end[b]]) for b in range(len(kinds))]
        _MESHES[key] = (verts, faces, v_start, f_start, fc.tolist(), per)
    return _MESHES[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- 1. sc_texture_queries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TEXELS)
@pytest.mark.parametrize("kinds,S", [("eab", 16), ("aeb", 16), ("abe", 16), ("e", 16), ("2", 32)])
def test_queries_bit_for_bit(kinds, S, T):
    """Positions and face indices of every texel of rows [0, rows), unused texels included, against numpy; the rows behind an image's
    texels (image_stride > rows A) and the memory behind both outputs keep their sentinel."""
    from shapeclipper_amd import _lib, ops
    verts, faces, v_start, f_start, F, per = _mesh(kinds, S)
    B = len(kinds)
    A, n, rows = ref.layout(max(F), T)
    assert tuple(ops.texture_layout(max(F), T)) == (A, n, rows)
    if kinds == "2":
        assert A > 64 and max(F) > 2 * (64 // T) ** 2
    if rows == 0:                                       # nothing holds a face: nothing to query
        q, fot = ops.texture_queries(verts, faces, v_start, f_start, F, A, T, LO, HI, S, rows)
        assert q.shape == (0, 3) and fot.shape == (B, 0)
        return
    extra, tail = 32, 64
    stride = rows * A + extra
    q = torch.full((B * stride + tail, 3), -7.0, device=DEV)
    fot = torch.full((B * rows * A + tail,), -7, dtype=torch.int32, device=DEV)
    starts = torch.tensor([v_start, f_start, F], dtype=torch.int64, device=DEV)
    code = _lib.load().sc_texture_queries(_lib.ptr(verts), _lib.ptr(faces), _lib.ptr(starts[0]), _lib.ptr(starts[1]), _lib.ptr(starts[2]),
                                          B, verts.shape[0], faces.shape[0], A, T, LO, HI, S, rows, stride, _lib.ptr(q), _lib.ptr(fot),
                                          _lib.stream())
    assert code == 0
    q_host, fot_host = q.cpu().numpy(), fot.cpu().numpy()
    assert (q_host[B * stride:] == -7).all() and (fot_host[B * rows * A:] == -7).all()
    blocks = q_host[:B * stride].reshape(B, stride, 3)
    assert (blocks[:, rows * A:] == -7).all()
    for b in range(B):
        want_q, want_f = ref.queries(*per[b], A, T, LO, HI, S, rows)
        assert np.array_equal(fot_host[b * rows * A:(b + 1) * rows * A], want_f), (kinds, b)
        assert np.array_equal(_bits(blocks[b, :rows * A]), _bits(want_q)), (kinds, b)
        assert (want_f >= 0).sum() == F[b] // 2 * T * T + (F[b] % 2) * (T * (T + 1) // 2)
        if F[b] == 0:
            assert (blocks[b, :rows * A] == np.float32(LO)).all()
    # the public form: the same bits in the padded layout, the extra rows left to the caller
    q2, fot2 = ops.texture_queries(verts, faces, v_start, f_start, F, A, T, LO, HI, S, rows, extra=16)
    assert q2.shape == (B * (rows * A + 16), 3) and fot2.shape == (B, rows * A)
    assert torch.equal(q2.view(B, -1, 3)[:, :rows * A], q[:B * stride].view(B, stride, 3)[:, :rows * A])
    assert torch.equal(fot2.view(-1), fot[:B * rows * A])


def test_queries_refusals():
    from shapeclipper_amd import ops
    verts, faces, v_start, f_start, F, _ = _mesh("ab")
    A, _, rows = ref.layout(max(F), 8)
    ok = lambda **kw: ops.texture_queries(verts, faces, kw.get("v", v_start), kw.get("f", f_start), kw.get("c", F), kw.get("A", A),
                                          kw.get("T", 8), LO, HI, kw.get("S", 16), kw.get("rows", rows))
    ok()
    for bad in (dict(A=96), dict(A=32), dict(T=3), dict(T=33), dict(S=1), dict(rows=rows + 1), dict(rows=A + 8), dict(rows=rows - 8),
                dict(f=[0, faces.shape[0]]), dict(c=[F[0], F[1] + 1]), dict(v=[0, verts.shape[0] + 1]), dict(c=F[:1])):
        with pytest.raises(ValueError):
            ok(**bad)


# ---- 2. layout -> texture coordinates -> look-up ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TEXELS)
def test_round_trip_against_float64(T):
    """The atlas holds the fp32 query positions themselves; the look-up at sum b_k vt_k of 4,096 random strictly interior barycentric
    points per image must give lo + (sum b_k v_k)(hi - lo) / (S - 1) as float64 evaluates it.

    Bound: k 2^-24 M E, M = max(|lo|, |hi|) the largest coordinate, E = (T-1)/(T-3) the largest extrapolation factor (every texel value
    and every barycentric coefficient is at most E times its in-triangle bound).  k counts the roundings of the header's op sequence,
    each at most 2^-24 of the quantity it rounds:
      texel value: b1, b2, 1 - b1, (.) - b2, three products, two sums, the product by scale and scale's own rounding are 11 roundings of
        quantities in grid-index units, at most E (S-1), which the scale turns into E (hi - lo) = 2 M E: 22;  (float)lo and the final
        addition round quantities of at most M E: 2;
      look-up: 1 - fx and 1 - fy (2), the two products and the sum of a row (3, the two rows combine with weights that sum to 1), the two
        row products and the last sum (3), and fx, fy themselves where x < 0 at the atlas edge (2): 10;
      texture coordinate: rounding u (and v) to fp32 and rounding u A - 0.5 each move the look-up by at most 2^-25 A texels, 2^-24 A per
        axis; a face of marching cubes lies in one grid cube, so a texel step changes a coordinate by at most one grid pitch / (T-3)
        = 2 M / ((S-1)(T-3)): ceil(4 A / ((S-1)(T-3))) for both axes.
    k = 34 + ceil(4 A / ((S-1)(T-3))): 69 at T = 4 (A = 128), 69 at T = 5 (A = 256), 48 at T = 8 (A = 256) on the S = 16 batch, 48 on the
    two spheres at S = 32, T = 8 (A = 512).  Measured worst case, in units of 2^-24 M E: 7.2 (T = 4), 9.0 (T = 5), 6.8 (T = 8) on the
    S = 16 batch; 5.9 on the two spheres.
    At the chart corners the look-up equals the corner texel -- the vertex's own query position -- bit for bit."""
    from shapeclipper_amd import ops
    from shapeclipper_amd.utils import eval_3D
    rng = np.random.RandomState(T)
    for kinds, S in (("aeb", 16), ("2", 32)):
        if S == 32 and T != 8:
            continue
        verts, faces, v_start, f_start, F, per = _mesh(kinds, S)
        B = len(kinds)
        A, n, rows = ref.layout(max(F), T)
        q, _ = ops.texture_queries(verts, faces, v_start, f_start, F, A, T, LO, HI, S, rows)
        atlas = torch.zeros(B, A, A, 3, device=DEV)
        atlas[:, :rows] = q.view(B, rows, A, 3)
        k = 34 + int(np.ceil(4 * A / ((S - 1) * (T - 3))))
        bound = k * 2.0 ** -24 * max(abs(LO), abs(HI)) * (T - 1) / (T - 3)
        worst = 0.0
        for b in range(B):
            if F[b] == 0:
                continue
            v, f = per[b]
            uv = ref.face_uv(F[b], A, T)                                        # float64, exact
            assert np.array_equal(eval_3D.texture_face_uv(F[b], A, T, DEV).cpu().numpy(), uv.astype(np.float32))
            pick = rng.randint(0, F[b], 4096)
            pick[:4] = (0, 1 % F[b], F[b] - 2, F[b] - 1)                        # first and last cell, both halves
            bary = np.maximum(rng.dirichlet((1.0, 1.0, 1.0), 4096), 1e-4)
            bary /= bary.sum(axis=1, keepdims=True)
            at = np.einsum("nk,nkc->nc", bary, uv[pick]).astype(np.float32)
            image = torch.full((4096,), b, dtype=torch.int32, device=DEV)
            got = ops.texture_sample(atlas, _dev(at), image).cpu().numpy().astype(np.float64)
            want = LO + np.einsum("nk,nkc->nc", bary, v[f[pick]].astype(np.float64)) * (HI - LO) / (S - 1)
            worst = max(worst, np.abs(got - want).max())
            # corners: exactly the corner texel = the vertex's query position
            corner = ops.texture_sample(atlas, _dev(uv.reshape(-1, 2).astype(np.float32)),
                                        torch.full((3 * F[b],), b, dtype=torch.int32, device=DEV)).cpu().numpy()
            vertex_q = np.float32(LO) + v[f.reshape(-1)] * ref.scale_of(LO, HI, S)
            assert np.array_equal(_bits(corner), _bits(vertex_q))
        print("round trip T=%d S=%d A=%d: worst |error| %.3e = %.2f x 2^-24 M E, bound k = %d (%.3e)"
              % (T, S, A, worst, worst / (bound / k), k, bound))
        assert worst <= bound


# ---- 3. sc_texture_sample --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "uint8"])
def test_sample_bit_for_bit(dtype):
    from shapeclipper_amd import ops
    rng = np.random.RandomState(3)
    for A, C, B in ((64, 3, 2), (128, 1, 1), (64, 4, 3)):
        if dtype == "fp32":
            atlas = rng.uniform(-2, 2, (B, A, A, C)).astype(np.float32)
        else:
            atlas = rng.randint(0, 256, (B, A, A, C)).astype(np.uint8)
        for N in (1, 63, 64, 65, 5000):
            uv = rng.uniform(-0.3, 1.3, (N, 2)).astype(np.float32)
            uv[::7] = rng.uniform(0, 1, uv[::7].shape)
            edge = np.array([[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.5 / A, 1 - 0.5 / A], [1 - 0.5 / A, 0.5 / A], [-50.0, 3e9], [1e30, -1e30]],
                            np.float32)
            uv[:min(N, len(edge))] = edge[:N]
            image = rng.randint(0, B, N).astype(np.int32)
            got = ops.texture_sample(_dev(atlas), _dev(uv), _dev(image))
            assert got.shape == (N, C) and got.dtype == torch.float32
            want = np.zeros((N, C), np.float32)
            for b in range(B):
                want[image == b] = ref.sample(atlas[b], uv[image == b])
            assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (A, C, N)
    with pytest.raises(ValueError):
        ops.texture_sample(torch.zeros(1, 96, 96, 3, device=DEV), torch.zeros(1, 2, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.texture_sample(torch.zeros(1, 64, 64, 3, device=DEV), torch.zeros(2, 3, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV))


def test_sample_writes_nothing_past_the_output():
    from shapeclipper_amd import _lib
    rng = np.random.RandomState(4)
    A, C, N = 64, 3, 65
    atlas, uv = _dev(rng.rand(1, A, A, C).astype(np.float32)), _dev(rng.rand(N, 2).astype(np.float32))
    image = torch.zeros(N, dtype=torch.int32, device=DEV)
    out = torch.full((N + 16, C), -7.0, device=DEV)
    assert _lib.load().sc_texture_sample(_lib.ptr(atlas), 0, _lib.ptr(uv), _lib.ptr(image), N, 1, A, C, _lib.ptr(out), _lib.stream()) == 0
    assert np.array_equal(_bits(out[:N].cpu().numpy()), _bits(ref.sample(atlas[0].cpu().numpy(), uv.cpu().numpy())))
    assert (out[N:] == -7).all()


# ---- 4. sc_texture_pack ----------------------------------------------------------------------------------------------------------------
def _networks(extra=(), seed=1):
    from shapeclipper_amd.model.implicit import RGBNetwork, SDFNetwork
    opt = _opt(["--eval.vox_res=16", *extra])
    torch.manual_seed(seed)
    sdf_net, rgb_net = SDFNetwork(opt), RGBNetwork(opt)
    with torch.no_grad():                                                       # (the SDF keeps its geometric init: a sphere)
        for p in rgb_net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return opt, sdf_net.to(DEV), rgb_net.to(DEV)


@pytest.mark.parametrize("T", TEXELS)
def test_pack_bytes(T):
    """The atlases' bytes against numpy, from the existing chain's outputs at the texels' queries: a used texel's colour is
    trunc(clamp(.) * 255) of ops.rgb_points_forward called here on the same queries; unused texels and the rows >= rows are 127."""
    from shapeclipper_amd import ops
    opt, sdf_net, rgb_net = _networks()
    kinds, S = "aeb", 16
    verts, faces, v_start, f_start, F, _ = _mesh(kinds, S)
    B = len(kinds)
    A, n, rows = ref.layout(max(F), T)
    q, fot = ops.texture_queries(verts, faces, v_start, f_start, F, A, T, LO, HI, S, rows)
    zs, zr = 0.1 * torch.randn(B, 64, device=DEV), torch.randn(B, 64, device=DEV)
    w_pack, cbias = sdf_net.packed(zs)
    v_pack, dbias = rgb_net.packed(zr)
    _, grad, feat = ops.sdf_forward(q, w_pack, cbias, rows * A, symmetric=bool(sdf_net.force_symmetry), want_grad=True, want_feat=True)
    rgb, normal = ops.rgb_points_forward(q, grad, feat, v_pack, dbias, rows * A, symmetric=bool(rgb_net.force_symmetry))
    atlas, atlas_n = ops.texture_pack(rgb, normal, fot, A, rows)
    assert atlas.shape == atlas_n.shape == (B, A, A, 3) and atlas.dtype == atlas_n.dtype == torch.uint8
    used = (fot >= 0).view(B, rows, A)
    quantised = (rgb.clamp(0, 1) * 255).to(torch.uint8).view(B, rows, A, 3)    # mesh_attributes' expression
    assert torch.equal(atlas[:, :rows][used], quantised[used])
    assert (atlas[:, :rows][~used] == 127).all() and (atlas[:, rows:] == 127).all()
    assert (atlas_n[:, :rows][~used] == 127).all() and (atlas_n[:, rows:] == 127).all()
    rgb_h, normal_h, fot_h = rgb.cpu().numpy().reshape(B, -1, 3), normal.cpu().numpy().reshape(B, -1, 3), fot.cpu().numpy()
    for b in range(B):
        want, want_n = ref.pack(rgb_h[b], normal_h[b], fot_h[b], A, rows)
        assert np.array_equal(atlas[b].cpu().numpy(), want) and np.array_equal(atlas_n[b].cpu().numpy(), want_n)
    assert (atlas[1] == 127).all() and len(torch.unique(atlas[0])) > 2         # the empty image; the other holds colours


def test_pack_clamps_and_fills():
    """Values outside [0, 1], exact byte boundaries and NaN, every texel used / none used / rows = 0 / rows = A."""
    from shapeclipper_amd import ops
    rng = np.random.RandomState(5)
    for A, rows in ((64, 0), (64, 8), (64, 64), (128, 40)):
        B = 2
        rgb = rng.uniform(-0.5, 1.5, (B, rows * A, 3)).astype(np.float32)
        nrm = rng.uniform(-1.5, 1.5, (B, rows * A, 3)).astype(np.float32)
        if rows:
            rgb[0, :6, 0] = (0.0, 1.0, np.nan, 127 / 255, 128 / 255, np.inf)
            nrm[0, :4, 1] = (-1.0, 1.0, np.nan, 0.0)
        fot = rng.randint(-1, 5, (B, rows * A)).astype(np.int32)
        fot[1] = -1 if rows != 64 else 3
        atlas, atlas_n = ops.texture_pack(_dev(rgb.reshape(-1, 3)), _dev(nrm.reshape(-1, 3)), _dev(fot), A, rows)
        for b in range(B):
            want, want_n = ref.pack(rgb[b], nrm[b], fot[b], A, rows)
            assert np.array_equal(atlas[b].cpu().numpy(), want) and np.array_equal(atlas_n[b].cpu().numpy(), want_n), (A, rows, b)
    with pytest.raises(ValueError):
        ops.texture_pack(torch.zeros(64 * 8, 3, device=DEV), torch.zeros(64 * 8, 3, device=DEV), torch.zeros(1, 64 * 8, dtype=torch.int32, device=DEV), 64, 16)


# ---- 5. eval_3D.mesh_texture -----------------------------------------------------------------------------------------------------------
def _bake_inputs(opt, sdf_net, B=3, seed=7):
    g = torch.Generator().manual_seed(seed)
    zs = (0.15 * torch.randn(B, 64, generator=g)).to(DEV)
    zr = torch.randn(B, 64, generator=g).to(DEV)
    level = _sphere_level(opt, sdf_net, zs)
    level[1] = 1.0                                                              # the middle image: no sign change, an empty mesh
    level[2] += 0.12                                                            # the last: a smaller solid, so fewer faces than the first
    return zs, zr, level


def _same(a, b):
    return (torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces) and torch.equal(a.uv, b.uv)
            and torch.equal(a.atlas, b.atlas) and torch.equal(a.normal_atlas, b.normal_atlas) and a.stats == b.stats)


def test_mesh_texture_against_float64():
    """The HIP path, three images (the middle one empty), T = 4: every used texel's colour within test_gpu_mesh_attributes' float64 budget
    (2e-5 before quantisation: at most one level apart) of the oracle's rgb_mlp at the texel's position, the normal atlas likewise within
    2e-4; the self-check is finite; the written vertices are those of {idx}_mesh.ply."""
    from oracle import reference_ops as R
    from shapeclipper_amd import ops
    from shapeclipper_amd.utils import eval_3D
    opt, sdf_net, rgb_net = _networks(["--eval.texture_texels=4"])
    zs, zr, level = _bake_inputs(opt, sdf_net)
    out = eval_3D.mesh_texture(opt, sdf_net, rgb_net, zs, zr, level)
    lo, hi = opt.eval.range
    S = level.shape[1]
    plain = eval_3D.meshes_device(level, lo, hi)
    verts, faces, vc, fc = ops.isosurface_mesh(level)
    F = fc.tolist()
    assert F[0] > 100 and F[2] > 100 and F[0] != F[2] and F[1] == 0
    A, n, rows = ref.layout(max(F), 4)
    v_end, f_end = np.cumsum(vc.numpy()).tolist(), np.cumsum(F).tolist()
    Ws = {k: v.detach().cpu() for k, v in sdf_net.weight_dict().items()}
    Wr = {k: v.detach().cpu() for k, v in rgb_net.weight_dict().items()}
    for b, m in enumerate(out):
        assert torch.equal(m.vertices, plain[b][0]) and torch.equal(m.faces, plain[b][1])
        if F[b] == 0:
            assert m.atlas.shape == (64, 64, 3) and (m.atlas == 127).all() and (m.normal_atlas == 127).all() and m.uv.shape == (0, 3, 2)
            assert m.stats == dict(faces=0, atlas=64, rows=0, err_mean=0.0, err_max=0.0)
            continue
        assert m.atlas.shape == m.normal_atlas.shape == (A, A, 3) and m.atlas.dtype == torch.uint8
        assert (m.stats["faces"], m.stats["atlas"], m.stats["rows"]) == (F[b], A, rows)
        assert np.isfinite(m.stats["err_mean"]) and np.isfinite(m.stats["err_max"]) and 0 <= m.stats["err_mean"] <= m.stats["err_max"] <= 255
        assert np.array_equal(m.uv.cpu().numpy(), ref.face_uv(F[b], A, 4).astype(np.float32))
        q, fot = ref.queries(verts[v_end[b] - int(vc[b]):v_end[b]].cpu().numpy(), faces[f_end[b] - F[b]:f_end[b]].cpu().numpy(), A, 4, lo, hi, S, rows)
        used = fot >= 0
        want_c, want_n = _reference(R.Cfg(), Ws, Wr, torch.from_numpy(q[used]), 1, zs[b:b + 1].cpu(), zr[b:b + 1].cpu())
        _check_quantised(m.atlas[:rows].reshape(-1, 3)[torch.from_numpy(used)], want_c)
        nb = m.normal_atlas[:rows].reshape(-1, 3)[torch.from_numpy(used)].cpu().double()
        t = ((want_n + 1) / 2).clamp(0, 1) * 255
        assert (nb <= t + 255 * 1e-4).all() and (nb > t - 1 - 255 * 1e-4).all()
        assert (m.atlas[:rows].reshape(-1, 3)[torch.from_numpy(~used)] == 127).all() and (m.atlas[rows:] == 127).all()
        print("mesh_texture image %d: F = %d, A = %d, rows = %d, centroid self-check mean %.3f max %.3f (of 255)"
              % (b, F[b], A, rows, m.stats["err_mean"], m.stats["err_max"]))


@pytest.mark.parametrize("T", TEXELS)
def test_mesh_texture_slabs_and_batches_change_no_byte(T, monkeypatch):
    """The slab size forced to 48 texels against the unforced single launch, for one image (48 per launch) and, at T = 4, for the batch of
    3 (16 per image and launch: every 16-point tile is a launch of its own); a slab that cuts every image's block of the batch a few
    times at every T; every image alone against the same image inside the batch wherever the batch's atlas is the image's own."""
    from shapeclipper_amd.utils import eval_3D
    opt, sdf_net, rgb_net = _networks(["--eval.texture_texels=%d" % T])
    zs, zr, level = _bake_inputs(opt, sdf_net)
    whole = eval_3D.mesh_texture(opt, sdf_net, rgb_net, zs, zr, level)
    from shapeclipper_amd import ops
    launches, forward = [], ops.sdf_forward
    monkeypatch.setattr(ops, "sdf_forward", lambda q, *a, **k: launches.append(q.shape[0]) or forward(q, *a, **k))
    one = eval_3D.mesh_texture(opt, sdf_net, rgb_net, zs[:1], zr[:1], level[:1], slab=48)
    monkeypatch.setattr(ops, "sdf_forward", forward)
    P = one[0].stats["rows"] * one[0].stats["atlas"] + 16 * -(-one[0].stats["faces"] // 16)      # the texels and the centroid block
    assert len(launches) == -(-P // 48) > 20 and max(launches) == 48 and sum(launches) == P and all(n % 16 == 0 for n in launches)
    assert _same(one[0], eval_3D.mesh_texture(opt, sdf_net, rgb_net, zs[:1], zr[:1], level[:1])[0])
    for slab in (3 * 16 * 331,) + ((48,) if T == 4 else ()):
        cut = eval_3D.mesh_texture(opt, sdf_net, rgb_net, zs, zr, level, slab=slab)
        assert all(_same(a, b) for a, b in zip(whole, cut)), slab
    alone = 0
    for b in range(3):
        single = eval_3D.mesh_texture(opt, sdf_net, rgb_net, zs[b:b + 1], zr[b:b + 1], level[b:b + 1])[0]
        if (single.stats["atlas"], single.stats["rows"]) == (whole[b].stats["atlas"], whole[b].stats["rows"]):
            assert _same(single, whole[b]), b
            alone += 1
        else:                                           # a smaller mesh than the batch's largest: the same charts in a larger atlas
            assert single.stats["faces"] == whole[b].stats["faces"] and torch.equal(single.vertices, whole[b].vertices)
    assert alone >= 2                                   # the largest image and the empty one


def test_mesh_texture_eager_path():
    """A compiled-family architecture (48 / 32 channels, 4 colour octaves) once on the HIP kernels and once on stock operators
    (sdf_network.eager): the two atlases within the float64 budget of each other's source, i.e. at most one level apart, and both
    self-checks finite."""
    from shapeclipper_amd.utils import eval_3D
    opt, sdf_net, rgb_net = _networks(["--eval.texture_texels=5", "--arch.impl_sdf.n_channels=48", "--arch.impl_rgb.n_channels=32",
                                       "--arch.impl_rgb.pos_enc=4"])
    assert not sdf_net.eager and not rgb_net.eager
    zs, zr, level = _bake_inputs(opt, sdf_net)
    hip = eval_3D.mesh_texture(opt, sdf_net, rgb_net, zs, zr, level)
    sdf_net.eager = rgb_net.eager = True
    try:
        eager = eval_3D.mesh_texture(opt, sdf_net, rgb_net, zs, zr, level, slab=3 * 4096)
    finally:
        sdf_net.eager = rgb_net.eager = False
    for a, b in zip(hip, eager):
        assert torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces) and torch.equal(a.uv, b.uv)
        assert a.atlas.shape == b.atlas.shape
        assert (a.atlas.int() - b.atlas.int()).abs().max().item() <= 1
        assert (a.normal_atlas.int() - b.normal_atlas.int()).abs().max().item() <= 1
        assert np.isfinite(b.stats["err_mean"]) and abs(a.stats["err_mean"] - b.stats["err_mean"]) <= 1.0
    assert hip[0].stats["faces"] > 100


# ---- 6. the evaluation's dumps ---------------------------------------------------------------------------------------------------------
def _parse_obj(path):
    out = dict(v=[], vt=[], f=[], mtllib=[], usemtl=[])
    for line in open(path).read().splitlines():
        key, *rest = line.split()
        if key in ("v", "vt"):
            out[key].append([float(x) for x in rest])
        elif key == "f":
            out["f"].append([[int(k) for k in c.split("/")] for c in rest])
        else:
            out[key].append(rest[0])
    return out


def _ply_vertices(fname):
    data = open(fname, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    n_v = int(data[:end].decode("ascii").splitlines()[2].split()[2])
    return np.frombuffer(data, "<f4", 3 * n_v, end).reshape(n_v, 3)


TEX_SUFFIXES = ("_mesh_tex.obj", "_mesh_tex.mtl", "_mesh_tex.png", "_mesh_tex_normal.png")


def test_evaluate_writes_textured_meshes(tmp_path):
    """Runner.evaluate (plain) and evaluate_sharded (combined with --hip.largest_component): with --eval.texture the four files per sample
    and texture.txt appear, the OBJ parses and its vertices are {idx}_mesh.ply's; without it every other file has the same bytes.  The
    vis_{ep}/ dump of the training-time visualisation goes through the same dump_geometry."""
    PIL = pytest.importorskip("PIL.Image")
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    from shapeclipper_amd.model.runner import Runner
    from shapeclipper_amd.utils import eval_3D
    from shapeclipper_amd.utils.util import EasyDict as edict
    o = _opt(["--arch.enc_pretrained!", "--data.dataset=synthetic", "--eval.vox_res=16", "--eval.num_points=1000", "--tb!", "--eval.texture"],
             output_root=str(tmp_path))
    o.device, o.world_size, o.port = 0, 1, 0
    torch.manual_seed(0)
    r = Runner(o)
    r.load_dataset(o, eval_split="test")
    r.build_networks(o)
    out = os.path.join(o.output_path, "dump")

    def snapshot():
        files = {os.path.join("dump", f): open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}
        files.update({f: open(os.path.join(o.output_path, f), "rb").read() for f in sorted(os.listdir(o.output_path)) if f.endswith(".txt")})
        return files

    def clear():
        for f in os.listdir(out) if os.path.isdir(out) else []:
            os.remove(os.path.join(out, f))
        for f in os.listdir(o.output_path):
            if f.endswith(".txt"):
                os.remove(os.path.join(o.output_path, f))

    is_new = lambda name: name == "texture.txt" or name.endswith(TEX_SUFFIXES)
    n_samples = len(r.test_data)
    for mode, largest in (("evaluate", False), ("evaluate_sharded", True)):
        o.hip.largest_component = largest
        clear()
        o.eval.texture = True
        getattr(r, mode)(o, ep=0)
        on = snapshot()
        rows = [l.split() for l in on["texture.txt"].decode().splitlines()]
        assert [int(x[0]) for x in rows] == list(range(n_samples)) and all(len(x) == 6 for x in rows)
        n_faces = 0
        for x in rows:
            i, faces, atlas, n_rows = (int(v) for v in x[:4])
            err_mean, err_max = float(x[4]), float(x[5])
            assert np.isfinite(err_mean) and np.isfinite(err_max) and 0 <= err_mean <= err_max <= 255
            for suffix in TEX_SUFFIXES:
                assert os.path.join("dump", "%d%s" % (i, suffix)) in on
            obj = _parse_obj(os.path.join(out, "%d_mesh_tex.obj" % i))
            assert obj["mtllib"] == ["%d_mesh_tex.mtl" % i] and len(obj["f"]) == faces and len(obj["vt"]) == 3 * faces
            assert on[os.path.join("dump", "%d_mesh_tex.mtl" % i)].decode().splitlines()[-1] == "map_Kd %d_mesh_tex.png" % i
            png, png_n = (np.asarray(PIL.open(os.path.join(out, "%d_mesh_tex%s.png" % (i, s)))) for s in ("", "_normal"))
            assert png.shape == png_n.shape == (atlas, atlas, 3) and (png[n_rows:] == 127).all()
            if faces == 0:
                assert atlas == 64 and n_rows == 0 and err_mean == err_max == 0 and (png == 127).all()
                continue
            n_faces += faces
            idx = np.array(obj["f"])
            assert idx[..., 0].min() >= 1 and idx[..., 0].max() <= len(obj["v"]) and idx[..., 1].max() == 3 * faces
            uv = np.array(obj["vt"], np.float32).reshape(faces, 3, 2)
            assert np.array_equal(uv, ref.face_uv(faces, atlas, 8).astype(np.float32))
            if not eval_3D.HAVE_MESHING:
                assert np.array_equal(np.array(obj["v"], np.float32), _ply_vertices(os.path.join(out, "%d_mesh.ply" % i)))
            assert len(np.unique(png[:n_rows].reshape(-1, 3), axis=0)) > 2
        assert n_faces > 0, mode
        # the switch off: none of the new files, every other file byte-identical
        clear()
        o.eval.texture = False
        getattr(r, mode)(o, ep=0)
        off = snapshot()
        assert not any(is_new(os.path.basename(k)) for k in off)
        assert off == {k: v for k, v in on.items() if not is_new(os.path.basename(k))}
        assert ("components.txt" in off) == largest
    # vis_{ep}/ of --hip.train_vis: dump_geometry writes the same four files there
    o.eval.texture, o.hip.largest_component = True, False
    r.graph.eval()
    o.H, o.W = o.eval.image_size
    os.makedirs(os.path.join(o.output_path, "vis_3"), exist_ok=True)
    sample = r.test_data[0]
    batch = {k: ({kk: vv[None] for kk, vv in v.items()} if isinstance(v, dict) else torch.as_tensor(v)[None]) for k, v in sample.items()}
    with torch.no_grad():
        var = r.evaluate_batch(o, edict(batch), 0, 0, single_gpu=True)
        eval_3D.eval_metrics(o, var, r.graph.module.sdf_network, vis_only=True)
        r.dump_geometry(o, var, "vis_3")
    names = os.listdir(os.path.join(o.output_path, "vis_3"))
    assert all("%d%s" % (int(var.idx[0]), s) in names for s in TEX_SUFFIXES)
