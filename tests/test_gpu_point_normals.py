"""ops.knn_points / point_normals / normal_consistency (csrc/point_normals.hip) and `--eval.normals`.

knn_points bit for bit against the brute-force numpy restatement of tests/point_normals_ref.py (indices equal, distance bits equal) on a
uniform volume, a sphere surface, a cloud with 50 exact duplicates, one with a distant outlier (the scan fallback) and N == k, for k in
3, 8, 16, 32; a NaN point; point_normals against the float64 restatement given the same indices to two fp32 ulps at 1 (2.4e-7: the
restatement agrees with numpy.linalg.eigh to 1e-15, so the one fp32 rounding of the output dominates) wherever the eigen-gap
(l1 - l0) / l2 >= 1e-3; normal_consistency against numpy float64 to 1e-12; the same bits run to run / on a side stream / alone and in a
batch; the refusals and the raw C ABI; the evaluation's files on the pix3d_mini tree with the switch off and on."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import point_normals_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEV = torch.device("cuda:0")
_INT = {torch.float64: torch.int64, torch.float32: torch.int32, torch.int32: torch.int32}
TOL = 2.4e-7


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(t):
    return t.contiguous().view(_INT[t.dtype]).cpu()


def _same_bits(a, b, what=""):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
        assert torch.equal(_bits(x), _bits(y)), (what, k)


# ---- 1. k nearest neighbours, bit for bit ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clouds():
    """{name: (points [B,N,3] fp32, restated idx [B,N,32], restated dist [B,N,32])}: the restatement once, at k = 32; the k smallest keys
    of a smaller k are its first k columns."""
    named = {"volume": ref.volume(11, 1000, images=3), "sphere": ref.sphere(5, 2000)[None], "duplicates": ref.with_duplicates(7, 700)[None],
             "outlier": ref.with_outlier(9, 1000)[None]}
    out = {}
    for name, p in named.items():
        got = [ref.knn(q, 32) for q in p]
        out[name] = (p, np.stack([g[0] for g in got]), np.stack([g[1] for g in got]))
    return out


@pytest.mark.parametrize("k", [3, 8, 16, 32])
def test_knn_is_bit_identical_to_the_restatement(clouds, k):
    from shapeclipper_amd import ops
    for name, (p, want_idx, want_dist) in clouds.items():
        idx, dist = ops.knn_points(_dev(p), k)
        assert idx.dtype == torch.int32 and dist.dtype == torch.float32 and idx.shape == dist.shape == (p.shape[0], p.shape[1], k)
        idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
        bad_i, bad_d = int((idx != want_idx[..., :k]).sum()), int((dist.view(np.int32) != want_dist[..., :k].view(np.int32)).sum())
        print("k = %2d %-10s: %d of %d indices and %d distances differ" % (k, name, bad_i, idx.size, bad_d))
        assert bad_i == 0 and bad_d == 0, name
    dup = clouds["duplicates"][1][0]
    assert dup[699, :32].tolist()[:3] == [7, 650, 651]                  # equal distances resolve to the lower index
    # N == k: every row is the whole cloud
    p = ref.volume(13 + k, k)
    want_idx, want_dist = ref.knn(p, k)
    idx, dist = ops.knn_points(_dev(p[None]), k)
    assert np.array_equal(idx[0].cpu().numpy(), want_idx) and np.array_equal(dist[0].cpu().numpy().view(np.int32), want_dist.view(np.int32))
    assert sorted(idx[0, 0].tolist()) == list(range(k))


def test_a_nan_point_leaves_every_other_row_exact():
    from shapeclipper_amd import ops
    p = ref.volume(21, 600, images=2)
    p[1, 123] = np.float32([0.1, np.nan, -0.2])
    res = ops.point_normals(_dev(p), 8)
    idx, dist = res.idx.cpu().numpy(), res.dist.cpu().numpy()
    for b in range(2):
        want_idx, want_dist = ref.knn(p[b], 8)
        rows = np.arange(600) != 123 if b == 1 else np.ones(600, bool)
        assert np.array_equal(idx[b][rows], want_idx[rows]) and np.array_equal(dist[b][rows].view(np.int32), want_dist[rows].view(np.int32))
    assert not (idx[1][np.arange(600) != 123] == 123).any()             # a NaN distance sorts last
    assert np.isnan(dist[1, 123]).all()
    assert not res.normals[1, 123].any() and float(res.variation[1, 123]) == 0.0
    want, _, _ = ref.normals(p[0], idx[0])
    assert np.abs(res.normals[0].cpu().numpy() - want).max() <= TOL


# ---- 2. normals against the restatement ------------------------------------------------------------------------------------------------
def _compare_normals(name, p, k, max_excluded):
    from shapeclipper_amd import ops
    res = ops.point_normals(_dev(p[None]), k)
    assert isinstance(res, ops.PointNormals) and res.normals.shape == (1, len(p), 3) and res.variation.shape == (1, len(p))
    assert res.normals.dtype == res.variation.dtype == torch.float32
    idx = res.idx[0].cpu().numpy()
    want, want_var, lam = ref.normals(p, idx)
    got, got_var = res.normals[0].cpu().numpy(), res.variation[0].cpu().numpy()
    with np.errstate(all="ignore"):
        keep = (lam[:, 1] - lam[:, 0]) / lam[:, 2] >= 1e-3
    err = np.minimum(np.abs(got - want), np.abs(got + want)).max(axis=1)
    print("%s k = %d: %d of %d points excluded (eigen-gap < 1e-3), worst |n - r| %.3g, worst |variation difference| %.3g"
          % (name, k, int((~keep).sum()), len(p), err[keep].max(), np.abs(got_var - want_var)[keep].max()))
    assert (~keep).sum() <= max_excluded * len(p)
    assert err[keep].max() <= TOL
    assert np.abs(got_var - want_var)[keep].max() <= 1e-7               # variation < 1/3: two fp32 ulps there are 6e-8
    same_sign = np.abs(got - want).max(axis=1) <= TOL                   # the sign rule itself, away from a tie of the largest components
    srt = np.sort(np.abs(want), axis=1)
    assert same_sign[keep & (srt[:, 2] - srt[:, 1] > 1e-6)].all()
    return got, keep


def test_normals_match_the_restatement_given_the_same_indices():
    p = ref.sphere(5, 2000)
    got, keep = _compare_normals("sphere", p, 16, 0.0)
    assert keep.all()
    r = p.astype(np.float64) / np.linalg.norm(p.astype(np.float64), axis=1, keepdims=True)
    cos = np.abs((got * r).sum(axis=1))
    print("sphere: min |n . r| %.4f, mean %.4f" % (cos.min(), cos.mean()))
    assert cos.min() >= 0.99 and cos.mean() >= 0.999
    for k in (3, 8, 32):
        _compare_normals("volume", ref.volume(3, 1000), k, 0.01)
    q, axis = ref.cube_surface(5, 3000)
    got, _ = _compare_normals("cube", q, 16, 0.01)
    other = np.abs(q).copy()
    other[np.arange(3000), axis] = 0
    inner = other.max(axis=1) < 0.3
    assert np.abs(got[np.arange(3000), axis])[inner].min() >= 1 - 1e-6


def test_degenerate_neighbourhoods_get_zero_normals():
    from shapeclipper_amd import ops
    line = np.zeros((40, 3), np.float32)
    line[:, 0] = np.arange(40) * 0.25 - 3
    line[:, 1] = 0.5 * line[:, 0]
    same = np.tile(np.float32([0.3, -0.2, 0.7]), (40, 1))
    generic = ref.volume(2, 40)
    res = ops.point_normals(_dev(np.stack([line, generic, same])), 5)
    assert not res.normals[0].any() and not res.variation[0].any() and not res.normals[2].any() and not res.variation[2].any()
    assert bool((res.normals[1].norm(dim=1) > 0.99).all())
    # indices handed in: an index outside the cloud makes that row degenerate, with no read out of bounds
    idx = res.idx.clone()
    idx[1, 7, 2] = 40
    idx[1, 9, 0] = -1
    again = ops.point_normals(_dev(np.stack([line, generic, same])), 5, idx=idx)
    assert again.dist is None and again.idx is idx
    rows = [i for i in range(40) if i not in (7, 9)]
    assert not again.normals[1, 7].any() and not again.normals[1, 9].any() and float(again.variation[1, 7]) == 0.0
    assert torch.equal(_bits(again.normals[1, rows]), _bits(res.normals[1, rows]))


# ---- 3. normal consistency -------------------------------------------------------------------------------------------------------------
def test_normal_consistency_against_numpy():
    from shapeclipper_amd import ops
    rng = np.random.default_rng(4)
    unit = lambda x: (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)
    B, N, M = 3, 2500, 1030                                              # 3 and 2 chunks of 1,024, both with a ragged end
    n1, n2 = unit(rng.normal(size=(B, N, 3))), unit(rng.normal(size=(B, M, 3)))
    i1, i2 = rng.integers(0, M, (B, N)).astype(np.int32), rng.integers(0, N, (B, M)).astype(np.int32)
    acc, comp = ops.normal_consistency(_dev(n1), _dev(n2), _dev(i1), _dev(i2))
    assert acc.dtype == comp.dtype == torch.float64 and acc.shape == comp.shape == (B,)
    for b in range(B):
        a, c = ref.normal_consistency(n1[b], n2[b], i1[b], i2[b])
        print("image %d: acc %.15f (numpy %.15f), comp %.15f (numpy %.15f)" % (b, float(acc[b]), a, float(comp[b]), c))
        assert abs(float(acc[b]) - a) <= 1e-12 and abs(float(comp[b]) - c) <= 1e-12
        assert 0 <= float(acc[b]) <= 1 and 0 <= float(comp[b]) <= 1
    # an index outside its cloud: NaN for that image and that direction, the rest keep their bits
    bad = i1.copy()
    bad[1, 2000] = M
    acc2, comp2 = ops.normal_consistency(_dev(n1), _dev(n2), _dev(bad), _dev(i2))
    assert bool(torch.isnan(acc2[1])) and torch.equal(_bits(acc2[[0, 2]]), _bits(acc[[0, 2]])) and torch.equal(_bits(comp2), _bits(comp))
    bad = i2.copy()
    bad[2, 0] = -1
    acc3, comp3 = ops.normal_consistency(_dev(n1), _dev(n2), _dev(i1), _dev(bad))
    assert bool(torch.isnan(comp3[2])) and torch.equal(_bits(comp3[:2]), _bits(comp[:2])) and torch.equal(_bits(acc3), _bits(acc))


def test_identical_clouds_and_normals_give_exactly_one():
    """Exactly 1 needs normals whose squared length is exactly 1 in float64: the cube's face normals +-e_a (a sum of n ones is exact).
    PCA normals are unit to one fp32 rounding, so their self-consistency is 1 to 2.4e-7."""
    from shapeclipper_amd import ops
    q, axis = ref.cube_surface(5, 3000)
    n = np.zeros((1, 3000, 3), np.float32)
    n[0, np.arange(3000), axis] = np.where(np.arange(3000) % 2 == 0, 1.0, -1.0)
    own = _dev(np.arange(3000, dtype=np.int32)[None])
    acc, comp = ops.normal_consistency(_dev(n), _dev(n), own, own)
    assert float(acc[0]) == 1.0 and float(comp[0]) == 1.0
    acc, comp = ops.normal_consistency(_dev(n), _dev(-n), own, own)      # unoriented
    assert float(acc[0]) == 1.0 and float(comp[0]) == 1.0
    res = ops.point_normals(_dev(ref.sphere(5, 2000)[None]), 16)
    own = _dev(np.arange(2000, dtype=np.int32)[None])
    acc, comp = ops.normal_consistency(res.normals, res.normals, own, own)
    assert abs(float(acc[0]) - 1) <= TOL and torch.equal(_bits(acc), _bits(comp))


# ---- 4. the same bits ------------------------------------------------------------------------------------------------------------------
def test_same_bits_run_to_run_on_a_side_stream_and_in_any_batch():
    from shapeclipper_amd import ops
    p = _dev(np.stack([ref.volume(1, 1500), ref.sphere(2, 1500), ref.with_outlier(3, 1500)]))
    q = _dev(ref.volume(4, 3 * 1100).reshape(3, 1100, 3))

    def run(p, q):
        a, b = ops.point_normals(p, 16), ops.point_normals(q, 8)
        i1 = a.idx[:, :, 1].remainder(q.shape[1]).contiguous()
        i2 = b.idx[:, :, 1].contiguous()
        return (*a, *b, *ops.normal_consistency(a.normals, b.normals, i1, i2))

    first = run(p, q)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = run(p, q)
    again = run(p, q)
    torch.cuda.synchronize()
    _same_bits(first, other, "side stream")
    _same_bits(first, again, "run to run")
    for k in range(3):
        one = run(p[k:k + 1].contiguous(), q[k:k + 1].contiguous())
        _same_bits([f[k:k + 1] for f in first], one, "image %d alone" % k)


# ---- 5. refusals and the raw C ABI -----------------------------------------------------------------------------------------------------
def test_refusals():
    from shapeclipper_amd import ops
    p = _dev(ref.volume(1, 100, images=2))
    idx, _ = ops.knn_points(p, 8)
    n = torch.zeros(2, 100, 3, device=DEV)
    i = torch.zeros(2, 100, dtype=torch.int32, device=DEV)
    for bad in (2, 33, 0, -1, 8.0, True, None):
        with pytest.raises(ValueError, match="k in 3..32"):
            ops.knn_points(p, bad)
        with pytest.raises(ValueError, match="k in 3..32"):
            ops.point_normals(p, bad)
    with pytest.raises(ValueError, match="fewer than k"):
        ops.knn_points(p[:, :7].contiguous(), 8)
    with pytest.raises(TypeError):
        ops.knn_points(p.double(), 8)
    with pytest.raises(TypeError):
        ops.point_normals(p, 8, idx=idx.long())
    with pytest.raises(TypeError):
        ops.normal_consistency(n, n, i.long(), i)
    with pytest.raises(TypeError):
        ops.normal_consistency(n.double(), n, i, i)
    with pytest.raises(ValueError):
        ops.knn_points(p.view(-1, 3), 8)
    with pytest.raises(ValueError):
        ops.knn_points(p[..., :2].contiguous(), 8)
    with pytest.raises(ValueError):
        ops.point_normals(p, 8, idx=idx[:, :, :7].contiguous())
    with pytest.raises(ValueError):
        ops.point_normals(p, 8, idx=idx.cpu())
    with pytest.raises(ValueError):
        ops.normal_consistency(n, n[:1].contiguous(), i, i[:1].contiguous())          # mismatched B
    with pytest.raises(ValueError):
        ops.normal_consistency(n, n, i[:, :-1].contiguous(), i)
    with pytest.raises(ValueError):
        ops.normal_consistency(n, n.cpu(), i, i)
    with pytest.raises(ValueError, match="contiguous"):
        ops.knn_points(p.transpose(0, 1).contiguous().transpose(0, 1), 8)
    with pytest.raises(ValueError, match="contiguous"):
        ops.normal_consistency(n, n, i.t().contiguous().t(), i)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.knn_points(p.cpu(), 8)
    empty_idx, empty_dist = ops.knn_points(p[:0].contiguous(), 8)       # no image: nothing is launched
    assert empty_idx.shape == empty_dist.shape == (0, 100, 8)


def test_raw_c_abi():
    from shapeclipper_amd import _lib, ops
    lib = _lib.load()
    B, N, K = 2, 900, 16
    pts = _dev(np.stack([ref.volume(5, N), ref.with_outlier(6, N)]))
    nbytes = int(lib.sc_knn_workspace_bytes(B, N, K))
    assert nbytes > 0 and lib.sc_knn_workspace_bytes(0, N, K) == 0
    for args in ((B, N, 2), (B, N, 33), (B, K - 1, K), (65536, N, K)):
        assert lib.sc_knn_workspace_bytes(*args) == -1
    ws = torch.full((nbytes,), 0xA5, device=DEV, dtype=torch.uint8)     # contents irrelevant on entry
    idx = torch.full((B, N, K), -7, device=DEV, dtype=torch.int32)
    dist = torch.full((B, N, K), -7.0, device=DEV)
    p, st = _lib.ptr, _lib.stream
    assert lib.sc_knn_points(p(pts), B, N, K, p(ws), p(idx), p(dist), st()) == 0
    want = ops.point_normals(pts, K)
    assert torch.equal(idx, want.idx) and torch.equal(_bits(dist), _bits(want.dist))
    normals, variation = torch.full((B, N, 3), -7.0, device=DEV), torch.full((B, N), -7.0, device=DEV)
    assert lib.sc_point_normals(p(pts), p(idx), B, N, K, p(normals), p(variation), st()) == 0
    assert torch.equal(_bits(normals), _bits(want.normals)) and torch.equal(_bits(variation), _bits(want.variation))
    own = torch.arange(N, dtype=torch.int32, device=DEV).repeat(B, 1)
    acc, comp = torch.full((B,), -7.0, device=DEV, dtype=torch.float64), torch.full((B,), -7.0, device=DEV, dtype=torch.float64)
    ws2 = torch.full((int(lib.sc_icp_workspace_bytes(B, N, N)),), 0xA5, device=DEV, dtype=torch.uint8)
    assert lib.sc_normal_consistency(p(normals), p(normals), p(own), p(own), B, N, N, p(ws2), p(acc), p(comp), st()) == 0
    _same_bits((acc, comp), ops.normal_consistency(want.normals, want.normals, own, own))
    # n_images <= 0 and refused arguments launch nothing: the outputs keep their fill
    idx2, dist2 = torch.full_like(idx, -7), torch.full_like(dist, -7.0)
    n2, v2, a2, c2 = torch.full_like(normals, -7.0), torch.full_like(variation, -7.0), torch.full_like(acc, -7.0), torch.full_like(comp, -7.0)
    for n_images in (0, -1):
        assert lib.sc_knn_points(p(pts), n_images, N, K, p(ws), p(idx2), p(dist2), st()) == 0
        assert lib.sc_point_normals(p(pts), p(idx), n_images, N, K, p(n2), p(v2), st()) == 0
        assert lib.sc_normal_consistency(p(normals), p(normals), p(own), p(own), n_images, N, N, p(ws2), p(a2), p(c2), st()) == 0
    for k_bad, n_bad, b_bad in ((2, N, B), (33, N, B), (K, K - 1, B), (K, N, 65536)):
        assert lib.sc_knn_points(p(pts), b_bad, n_bad, k_bad, p(ws), p(idx2), p(dist2), st()) == 1
        assert lib.sc_point_normals(p(pts), p(idx), b_bad, n_bad, k_bad, p(n2), p(v2), st()) == 1
    assert lib.sc_knn_points(None, B, N, K, p(ws), p(idx2), p(dist2), st()) == 1
    assert lib.sc_knn_points(p(pts), B, N, K, None, p(idx2), p(dist2), st()) == 1
    assert lib.sc_knn_points(p(pts), B, N, K, p(ws), None, p(dist2), st()) == 1
    assert lib.sc_knn_points(p(pts), B, N, K, p(ws), p(idx2), None, st()) == 1
    assert lib.sc_point_normals(p(pts), None, B, N, K, p(n2), p(v2), st()) == 1
    assert lib.sc_point_normals(p(pts), p(idx), B, N, K, p(n2), None, st()) == 1
    assert lib.sc_normal_consistency(p(normals), None, p(own), p(own), B, N, N, p(ws2), p(a2), p(c2), st()) == 1
    assert lib.sc_normal_consistency(p(normals), p(normals), p(own), p(own), B, N, N, None, p(a2), p(c2), st()) == 1
    assert lib.sc_normal_consistency(p(normals), p(normals), p(own), p(own), B, 0, N, p(ws2), p(a2), p(c2), st()) == 1
    assert lib.sc_normal_consistency(p(normals), p(normals), p(own), p(own), 65536, N, N, p(ws2), p(a2), p(c2), st()) == 1
    torch.cuda.synchronize()
    for t in (idx2, dist2, n2, v2, a2, c2):
        assert bool((t == -7).all())


# ---- 5b. the prediction's normals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ["shipped", "eager"])
def test_predicted_normals_against_float64(tmp_path, arch):
    """eval_3D.predicted_normals on the compiled SDF family (HIP) and on a 6 x 128 network (stock operators): the unit float64 gradient of
    the reference network at lo + (p - lo) S / (S - 1), to the 2e-4 that tests/test_gpu_mesh_attributes.py holds the same kernel's
    normals to.  N = 1,000 is no multiple of 16 (8 padding rows per image), B = 2."""
    from oracle import reference_ops as R
    from shapeclipper_amd.model.implicit import SDFNetwork
    from shapeclipper_amd.utils import eval_3D, options
    extra = [] if arch == "shipped" else ["--arch.impl_sdf.n_hidden_layers=6", "--arch.impl_sdf.n_channels=128"]
    opt = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_normals_net",
                                               "--output_root=%s" % tmp_path, "--eval.vox_res=16", *extra]), verbose=False)
    torch.manual_seed(2)
    net = SDFNetwork(opt)
    assert bool(net.eager) == (arch == "eager")
    net = net.to(DEV)
    B, N, S = 2, 1000, 17
    z = 0.1 * torch.randn(B, 64, device=DEV)
    pts = _dev(np.stack([ref.sphere(1, N, 0.4), ref.sphere(2, N, 0.3)]))
    got = eval_3D.predicted_normals(opt, net, z, pts, S)
    assert got.shape == (B, N, 3) and got.dtype == torch.float32 and got.is_contiguous()
    lo, _ = opt.eval.range
    q = (lo + (pts.cpu().double() - lo) * (S / (S - 1))).reshape(-1, 3)
    cfg = R.Cfg() if arch == "shipped" else R.Cfg(hidden_sdf=128, n_hidden_sdf=6)
    Ws = {k: v.detach().cpu().double() for k, v in net.weight_dict().items()}
    _, _, grad = R.sdf_conditional(cfg, Ws, B, q, z.cpu().double(), compute_grad=True)
    grad = grad.detach()
    want = (grad / grad.norm(dim=1, keepdim=True)).view(B, N, 3)
    err = (got.cpu().double() - want).abs().max().item()
    print("predicted_normals %s: worst |difference| from float64 %.3g" % (arch, err))
    assert err < 2e-4


# ---- 6. the evaluation on the pix3d_mini tree ------------------------------------------------------------------------------------------
NEW_FILES = ("normal_consistency.txt", "nc_cat.txt")
ICP_FILES = ("normal_consistency_icp.txt", "nc_cat_icp.txt")
NEW_KEYS = ("nc", "nc_acc", "nc_comp", "normals_pred")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from shapeclipper_amd.data import pix3d_mini
    root = str(tmp_path_factory.mktemp("pix3d_normals") / "Pix3D")
    pix3d_mini.write_tree(root, n_per_cat=6, k_nearest=5, cat_key="chair,sofa", n_points=2000, seed=11)
    return root


def _opt(tree, output_root, extra=()):
    from shapeclipper_amd.utils import options
    o = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_normals", "--output_root=%s" % output_root,
                                             "--arch.enc_pretrained!", "--tb!", "--batch_size=2", "--data.pix3d.cat=chair,sofa",
                                             "--data.num_classes=2", "--data.pix3d.root=%s" % tree, "--data.num_workers=0",
                                             "--data.max_img_cat=2", "--eval.vox_res=16", "--eval.num_points=1000", *extra]), verbose=False)
    o.device, o.world_size, o.port = 0, 1, 0
    return o


def _runner(o):
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    from shapeclipper_amd.model.runner import Runner
    torch.manual_seed(0)
    r = Runner(o)
    r.load_dataset(o, eval_split="test")
    r.build_networks(o)
    r.graph.eval()
    return r


def _box_grid(o):
    """A level grid whose solid is the box |x| < .3, |y| < .2, |z| < .25, at get_dense_3D_grid's positions."""
    lo, hi = o.eval.range
    g = torch.linspace(lo, hi, o.eval.vox_res + 1, device=DEV)
    pts = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), dim=-1)
    return (pts.abs() - torch.tensor([0.3, 0.2, 0.25], device=DEV)).amax(dim=-1).contiguous()


def _sample_var(r, o, it=0):
    from shapeclipper_amd.utils.util import EasyDict as edict
    sample = r.test_data[it]
    batch = {k: ({kk: vv[None] for kk, vv in v.items()} if isinstance(v, dict) else torch.as_tensor(v)[None]) for k, v in sample.items()}
    o.H, o.W = o.eval.image_size
    with torch.no_grad():
        return r.evaluate_batch(o, edict(batch), 0, it, single_gpu=True)


def _files(o):
    """{relative name: bytes} of the .txt files of the output folder and of every per-sample file under dump/."""
    out = {}
    for folder in ("", "dump"):
        d = os.path.join(o.output_path, folder)
        for f in sorted(os.listdir(d)) if os.path.isdir(d) else []:
            if os.path.isfile(os.path.join(d, f)) and (folder or f.endswith(".txt")):
                out[os.path.join(folder, f)] = open(os.path.join(d, f), "rb").read()
    return out


def _read_ply(data, with_normals):
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n_v = int([l for l in lines if l.startswith("element vertex")][0].split()[2])
    names = ("x", "y", "z", "nx", "ny", "nz") if with_normals else ("x", "y", "z")
    assert [l.split()[2] for l in lines if l.startswith("property")] == list(names) + ["red", "green", "blue"]
    vdt = np.dtype([(k, "<f4") for k in names] + [(k, "u1") for k in ("red", "green", "blue")])
    assert end + vdt.itemsize * n_v == len(data)
    return np.frombuffer(data, vdt, n_v, end)


def test_evaluation_writes_the_normal_files_beside_the_raw_ones(tree, tmp_path, monkeypatch):
    import chamfer_3D
    from shapeclipper_amd import ops
    from shapeclipper_amd.utils import eval_3D
    o = _opt(tree, str(tmp_path))
    assert "normals" not in o.eval
    r = _runner(o)
    grid = _box_grid(o)
    monkeypatch.setattr(eval_3D, "HAVE_MESHING", False)
    monkeypatch.setattr(eval_3D, "compute_level_grid", lambda opt, net, z, pts: grid[None].repeat(pts.shape[0], 1, 1, 1))
    n = len(r.test_data)
    assert n == 4
    net = r.graph.module.sdf_network

    # ---- off: nothing new, in the files or in var; the loader's normals stay zero ----
    raw_value = r.evaluate(o, ep=0)
    off = _files(o)
    assert not any("normal" in f or "nc_" in f for f in off), sorted(off)
    assert {"chamfer.txt", "cd_cat.txt", "f_score.txt"} <= set(off)
    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net)
    assert not any(k in var for k in NEW_KEYS) and "variation" not in var.dpc and not var.dpc.normals.any()
    raw = (var.cd_acc.clone(), var.cd_comp.clone(), var.f_score.clone(), var.dpc_pred.clone(), var.dpc.points.clone())

    # ---- on ----
    o.eval.normals = True
    assert r.evaluate(o, ep=0) == raw_value                             # the returned value is the raw one
    on = _files(o)
    for f, data in off.items():
        assert on[f] == data, f                                         # every existing output keeps its bytes
    ply = ["dump/%d_pointclouds_normals.ply" % i for i in range(n)]
    assert sorted(set(on) - set(off)) == sorted(list(NEW_FILES) + ply)
    lines = [l.split() for l in on["normal_consistency.txt"].decode().splitlines()]
    assert [int(l[0]) for l in lines] == [int(l.split()[0]) for l in on["chamfer.txt"].decode().splitlines()] == list(range(n))
    for l in lines:
        print("normal_consistency.txt:", " ".join(l))
        assert len(l) == 4 and all(len(x.split(".")[1]) == 8 for x in l[1:])
        acc, comp, nc = (float(x) for x in l[1:])
        assert 0 <= acc <= 1 and 0 <= comp <= 1 and abs(nc - (acc + comp) / 2) <= 1e-8
    cat = on["nc_cat.txt"].decode().splitlines()
    assert cat[0] == "NC     Acc    Comp   Count Cat" and len(cat) == len(on["cd_cat.txt"].splitlines())
    assert [l.split()[3:] for l in cat[1:]] == [l.split()[3:] for l in on["cd_cat.txt"].decode().splitlines()[1:]]
    assert all(0 <= float(x) <= 1 for l in cat[1:] for x in l.split()[:3])

    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net)
    assert all(k in var for k in NEW_KEYS) and not any(k.endswith("_icp") for k in var)
    for a, b in zip(raw, (var.cd_acc, var.cd_comp, var.f_score, var.dpc_pred, var.dpc.points)):
        assert torch.equal(a, b)                                        # the raw metrics are computed exactly as before
    assert var.nc.dtype == torch.float64 and var.nc.shape == var.nc_acc.shape == var.nc_comp.shape == (1,)
    assert var.normals_pred.shape == (1, 1000, 3) and var.dpc.normals.shape == var.dpc.points.shape == (1, 2000, 3)
    length = var.dpc.normals.double().norm(dim=-1)
    assert bool(((length - 1).abs() <= 1e-6)[var.dpc.variation > 0].all()) and bool((var.dpc.variation > 0).any())
    assert bool(((var.normals_pred.double().norm(dim=-1) - 1).abs() <= 1e-5).all())

    # ---- the same numbers from the ops chained by hand ----
    lo, hi = o.eval.range
    S = o.eval.vox_res + 1
    pts, _ = eval_3D.surface_points_device(var.level_vox, lo, hi, 1000, seed=int(var.idx[0]))
    q = lo + (pts - lo) * (S / (S - 1))
    query = torch.cat([q, q[:, :1].expand(1, 8, 3)], dim=1).reshape(-1, 3).contiguous()              # 1000 -> 1008 rows, a multiple of 16
    w_pack, cbias = net.packed(var.proj_latent_sdf)
    _, grad, _ = ops.sdf_forward(query, w_pack, cbias, 1008, symmetric=bool(net.force_symmetry), want_grad=True, want_feat=False)
    normal = torch.nn.functional.normalize(grad, dim=1, eps=1e-12).view(1, 1008, 3)[:, :1000].contiguous()
    normal = (var.pose[..., :3] @ normal.permute(0, 2, 1)).permute(0, 2, 1).contiguous()
    flip = torch.tensor(eval_3D._FLIP_PRED, device=DEV).float()[None]
    normal = (flip @ normal.permute(0, 2, 1)).permute(0, 2, 1).contiguous()
    assert torch.equal(_bits(normal), _bits(var.normals_pred))
    gt = ops.point_normals(var.dpc.points.contiguous(), 16)
    assert torch.equal(_bits(gt.normals), _bits(var.dpc.normals)) and torch.equal(_bits(gt.variation), _bits(var.dpc.variation))
    d1, d2 = torch.zeros(1, 1000, device=DEV), torch.zeros(1, 2000, device=DEV)
    i1, i2 = torch.zeros(1, 1000, dtype=torch.int32, device=DEV), torch.zeros(1, 2000, dtype=torch.int32, device=DEV)
    chamfer_3D.forward(var.dpc_pred.contiguous(), var.dpc.points.contiguous(), d1, d2, i1, i2)
    acc, comp = ops.normal_consistency(normal, gt.normals, i1, i2)
    assert torch.equal(_bits(acc), _bits(var.nc_acc)) and torch.equal(_bits(comp), _bits(var.nc_comp))
    assert torch.equal(_bits((acc + comp) / 2), _bits(var.nc))
    assert lines[0] == ("0 %.8f %.8f %.8f" % (float(acc), float(comp), float((acc + comp) / 2))).split()
    v = _read_ply(on[ply[0]], True)
    both = _read_ply(on["dump/0_pointclouds_comp.ply"], False)
    assert len(v) == len(both) == 3000 and all(np.array_equal(v[k], both[k]) for k in ("x", "y", "z", "red", "green", "blue"))
    assert np.array_equal(np.stack([v["nx"], v["ny"], v["nz"]], 1), torch.cat([var.normals_pred[0], var.dpc.normals[0]]).cpu().numpy())

    # ---- the sharded evaluation writes the same lines from its extra gather ----
    for f in NEW_FILES:
        os.remove(os.path.join(o.output_path, f))
    assert r.evaluate_sharded(o, ep=0) == pytest.approx(raw_value, rel=1e-5)
    sharded = _files(o)
    assert set(sharded) == set(on)
    if sharded["chamfer.txt"] == on["chamfer.txt"]:
        assert sharded["normal_consistency.txt"] == on["normal_consistency.txt"] and sharded["nc_cat.txt"] == on["nc_cat.txt"]
    else:
        print("evaluate and evaluate_sharded differ on chamfer.txt: normal_consistency.txt not compared")
    assert [int(l.split()[0]) for l in sharded["normal_consistency.txt"].decode().splitlines()] == list(range(n))

    # ---- with --eval.icp: the _icp namesakes, from the last ICP search and the rotated normals ----
    o.eval.icp = True
    o.eval.icp_iters = 6
    assert r.evaluate(o, ep=0) == raw_value
    both_on = _files(o)
    for f, data in on.items():
        assert both_on[f] == data, f
    assert set(ICP_FILES) <= set(both_on) - set(on)
    icp_lines = [l.split() for l in both_on["normal_consistency_icp.txt"].decode().splitlines()]
    assert [int(l[0]) for l in icp_lines] == list(range(n)) and all(0 <= float(x) <= 1 for l in icp_lines for x in l[1:])
    assert both_on["nc_cat_icp.txt"].decode().splitlines()[0] == cat[0]
    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net)
    assert torch.equal(_bits(var.nc), _bits((acc + comp) / 2))
    res = ops.icp_align(var.dpc_pred.contiguous(), var.dpc.points.contiguous(), iters=6, scale=True)
    R = res.transform[:, :3, :3] / res.s[:, None, None]
    rotated = (R @ var.normals_pred.double().permute(0, 2, 1)).permute(0, 2, 1).contiguous().float()
    assert torch.equal(_bits(rotated), _bits(var.normals_pred_icp))
    acc_i, comp_i = ops.normal_consistency(rotated, var.dpc.normals, res.idx1, res.idx2)
    assert torch.equal(_bits(acc_i), _bits(var.nc_acc_icp)) and torch.equal(_bits(comp_i), _bits(var.nc_comp_icp))
    assert icp_lines[0] == ("0 %.8f %.8f %.8f" % (float(acc_i), float(comp_i), float(var.nc_icp))).split()
    for f in NEW_FILES + ICP_FILES:
        os.remove(os.path.join(o.output_path, f))
    r.evaluate_sharded(o, ep=0)
    sharded = _files(o)
    assert set(sharded) == set(both_on)
    if sharded["chamfer.txt"] == both_on["chamfer.txt"]:
        assert sharded["normal_consistency_icp.txt"] == both_on["normal_consistency_icp.txt"]
        assert sharded["nc_cat_icp.txt"] == both_on["nc_cat_icp.txt"]

    # ---- vis_only skips it ----
    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net, vis_only=True)
    assert not any(k in var for k in NEW_KEYS)
