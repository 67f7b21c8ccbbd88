"""ops.icp_fit / icp_apply / icp_align (csrc/icp.hip around the Chamfer search) and `--eval.icp`.

icp_fit against the float64 numpy restatement of tests/icp_ref.py given the same indices (1e-9 absolute: both are float64 and differ in
summation order and SVD method only; N 2^-53 10 is about 1e-12), its degenerate rules, icp_apply bit for bit, recovery of the known
transform of the 16 chair cases to 2e-8 (ten times the restatement's worst), a monotone objective, the same bits run to run / on a side
stream / alone and in a batch / against a hand-chained loop, the refusals, and the evaluation's files with the switch off and on."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FIELDS = ("transform", "s", "aligned", "dist1", "dist2", "idx1", "idx2", "objective")
_INT = {torch.float64: torch.int64, torch.float32: torch.int32, torch.int32: torch.int32}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(t):
    return t.contiguous().view(_INT[t.dtype]).cpu()


def _same_bits(a, b, what=""):
    for name, x, y in zip(FIELDS, a, b):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name)
        assert torch.equal(_bits(x), _bits(y)), (what, name)


def _search(cur, dst):
    import chamfer_3D
    B, N, M = cur.shape[0], cur.shape[1], dst.shape[1]
    d1, d2 = torch.zeros(B, N, device=DEV), torch.zeros(B, M, device=DEV)
    i1, i2 = torch.zeros(B, N, dtype=torch.int32, device=DEV), torch.zeros(B, M, dtype=torch.int32, device=DEV)
    chamfer_3D.forward(cur, dst, d1, d2, i1, i2)
    return d1, d2, i1, i2


# ---- 1. the fit ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generic():
    """Random generic clouds N = 1000, M = 1500, B = 3 in [-1, 1] and the search's own indices for them."""
    rng = np.random.default_rng(11)
    src = rng.uniform(-1, 1, (3, 1000, 3)).astype(np.float32)
    dst = rng.uniform(-1, 1, (3, 1500, 3)).astype(np.float32)
    _, _, i1, i2 = _search(_dev(src), _dev(dst))
    return src, dst, i1.cpu().numpy(), i2.cpu().numpy()


@pytest.mark.parametrize("scale", [True, False])
def test_fit_matches_the_restatement_given_the_same_indices(generic, scale):
    from shapeclipper_amd import ops
    src, dst, i1, i2 = generic
    T, s = ops.icp_fit(_dev(src), _dev(dst), _dev(i1), _dev(i2), scale=scale)
    assert T.dtype == torch.float64 and T.shape == (3, 4, 4) and s.dtype == torch.float64 and s.shape == (3,)
    T, s = T.cpu().numpy(), s.cpu().numpy()
    for b in range(3):
        Tr, sr = ref.fit(src[b], dst[b], i1[b], i2[b], scale=scale)
        err = max(np.abs(T[b] - Tr).max(), abs(s[b] - sr))
        print("scale=%s image %d: worst |entry difference| %.3g, s = %.12f" % (scale, b, err, s[b]))
        assert err <= 1e-9
        assert np.array_equal(T[b, 3], [0, 0, 0, 1])
        assert scale or s[b] == 1.0
        R = T[b, :3, :3] / s[b]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and np.linalg.det(R) > 0


def test_degenerate_images_get_the_identity_and_leave_the_others_alone(generic):
    from shapeclipper_amd import ops
    src, dst, i1, i2 = generic
    want, want_s = ops.icp_fit(_dev(src), _dev(dst), _dev(i1), _dev(i2))
    same = np.tile(np.float32([0.3, -0.2, 0.7]), (1000, 1))
    line = np.float32([0.25, -0.5, 0.125]) + np.arange(-500, 500, dtype=np.float32)[:, None] * np.float32([2 ** -11, 2 ** -10, -2 ** -11])
    nan = src[1].copy()
    nan[123, 2] = np.nan
    for name, bad in (("all source points equal", same), ("collinear", line), ("one NaN coordinate", nan)):
        s2 = src.copy()
        s2[1] = bad
        T, s = ops.icp_fit(_dev(s2), _dev(dst), _dev(i1), _dev(i2))
        assert torch.equal(T[1].cpu(), torch.eye(4, dtype=torch.float64)) and float(s[1]) == 1.0, name
        for b in (0, 2):
            assert torch.equal(_bits(T[b]), _bits(want[b])) and torch.equal(_bits(s[b]), _bits(want_s[b])), name
    # an index outside its cloud is a NaN pair, not a read out of bounds
    bad_idx = i1.copy()
    bad_idx[2, 5] = 1500
    T, s = ops.icp_fit(_dev(src), _dev(dst), _dev(bad_idx), _dev(i2))
    assert torch.equal(T[2].cpu(), torch.eye(4, dtype=torch.float64)) and torch.equal(_bits(T[:2]), _bits(want[:2]))


# ---- 2. the apply ----------------------------------------------------------------------------------------------------------------------
def test_apply_is_bit_identical_to_the_restatement():
    from shapeclipper_amd import ops
    rng = np.random.default_rng(3)
    src = rng.uniform(-1, 1, (4, 1000, 3)).astype(np.float32)
    src[3] *= np.float32(1e3)
    T = np.tile(np.eye(4), (4, 1, 1))
    T[0, :3, :3] = 1.1 * ref.rotation((1, 2, 3), 10.0); T[0, :3, 3] = (0.05, -0.02, 0.01)
    T[1, :3, :3] = rng.normal(size=(3, 3)); T[1, :3, 3] = (1.0e6, -3.0e5, 7.0e6 + 0.123)           # a large t
    T[3, :3, :3] = 0.9 * ref.rotation((-1, 0.5, 0.2), 33.0); T[3, :3, 3] = (1e-3, 2e-3, -5.0)
    out = ops.icp_apply(_dev(src), _dev(T))
    assert out.dtype == torch.float32 and out.shape == (4, 1000, 3)
    got = out.cpu().numpy()
    for b in range(4):
        want = ref.apply(src[b], T[b])
        print("image %d: %d of %d values differ" % (b, int((got[b].view(np.int32) != want.view(np.int32)).sum()), want.size))
        assert np.array_equal(got[b].view(np.int32), want.view(np.int32))
    assert np.array_equal(got[2].view(np.int32), src[2].view(np.int32))                          # the identity returns the input's bits


# ---- 3. recovery, 4. monotone objective ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recovered():
    """[(case, IcpResult fields of that image as numpy)] of the 16 cases: the scaled ones in one call, the rigid ones in another."""
    from shapeclipper_amd import ops
    cases = ref.all_cases()
    out = [None] * len(cases)
    for scale in (True, False):
        sel = [k for k, c in enumerate(cases) if c["scale"] is scale]
        res = ops.icp_align(_dev(np.stack([cases[k]["src"] for k in sel])), _dev(np.stack([cases[k]["dst"] for k in sel])), iters=30, scale=scale)
        assert isinstance(res, ops.IcpResult) and res._fields == FIELDS
        host = [f.cpu().numpy() for f in res]
        for j, k in enumerate(sel):
            out[k] = (cases[k], {name: h[j] for name, h in zip(FIELDS, host)})
    return out


def _check_recovery(c, r, what):
    T, s = r["transform"], r["s"]
    err = max(np.abs(T[:3, :3] / s - c["R0"]).max(), np.abs(T[:3, 3] - c["t0"]).max(), abs(s - c["s0"]))
    print("%s: worst |error| of R, t, s = %.3g; objective %.3g -> %.3g" % (what, err, r["objective"][0], r["objective"][-1]))
    assert err <= 2e-8, what
    assert np.array_equal(r["idx1"], c["inv"]), what
    assert r["objective"][-1] <= 1e-12, what
    assert np.array_equal(r["aligned"].view(np.int32), ref.apply(c["src"], T).view(np.int32)), what


def test_recovers_the_known_transform_of_every_case(recovered):
    assert len(recovered) == 16
    for k, (c, r) in enumerate(recovered):
        assert r["objective"].shape == (31,) and r["transform"].shape == (4, 4)
        _check_recovery(c, r, "case %d (seed %d)" % (k % 4, k // 4))


def test_recovers_with_the_grid_search_in_the_loop_and_brute_gives_the_same_bits(monkeypatch):
    import chamfer_3D
    from shapeclipper_amd import ops
    c = ref.case(0, 0, n=4096)
    assert chamfer_3D.SEARCH == "grid" and chamfer_3D._path(4096, 4096) == "grid"
    src, dst = _dev(c["src"][None]), _dev(c["dst"][None])
    res = ops.icp_align(src, dst, iters=30, scale=True)
    _check_recovery(c, {name: f[0].cpu().numpy() for name, f in zip(FIELDS, res)}, "N = M = 4096")
    monkeypatch.setattr(chamfer_3D, "SEARCH", "brute")
    assert chamfer_3D._path(4096, 4096) == "split"
    _same_bits(res, ops.icp_align(src, dst, iters=30, scale=True), "grid against brute")


def _check_monotone(obj, what):
    worst = max(float(obj[j + 1] - obj[j] - (1e-5 * np.sqrt(obj[j]) + 1e-12)) for j in range(len(obj) - 1))
    print("%s: objective %.6g -> %.6g, largest (rise - slack) %.3g" % (what, obj[0], obj[-1], worst))
    for j in range(len(obj) - 1):
        assert obj[j + 1] <= obj[j] + 1e-5 * np.sqrt(obj[j]) + 1e-12, (what, j)
    assert obj[-1] < 0.5 * obj[0], what


def test_the_objective_never_rises(recovered):
    from shapeclipper_amd import ops
    for k, (_, r) in enumerate(recovered):
        _check_monotone(r["objective"], "case %d (seed %d)" % (k % 4, k // 4))
    src, dst = ref.unmatched_case()
    assert src.shape == (1024, 3) and dst.shape == (1500, 3)
    res = ops.icp_align(_dev(src[None]), _dev(dst[None]), iters=30, scale=True)
    _check_monotone(res.objective[0].cpu().numpy(), "no true correspondences")
    d1, d2, i1, i2 = _search(res.aligned, _dev(dst[None]))                                      # the result's fields are the last search's
    assert torch.equal(_bits(d1), _bits(res.dist1)) and torch.equal(i2, res.idx2)
    want = d1.double().mean() + d2.double().mean()
    assert abs(float(res.objective[0, -1]) - float(want)) <= 1e-12 * float(want)


# ---- 5. the same bits ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trio():
    cs = [ref.case(0, 0), ref.case(1, 1), ref.case(2, 3)]
    return _dev(np.stack([c["src"] for c in cs])), _dev(np.stack([c["dst"] for c in cs]))


def test_same_bits_run_to_run_on_a_side_stream_and_in_any_batch(trio):
    from shapeclipper_amd import ops
    src, dst = trio
    a = ops.icp_align(src, dst, iters=8)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b = ops.icp_align(src, dst, iters=8)
    c = ops.icp_align(src, dst, iters=8)
    torch.cuda.synchronize()
    _same_bits(a, b, "side stream")
    _same_bits(a, c, "run to run")
    for k in range(3):
        one = ops.icp_align(src[k:k + 1].contiguous(), dst[k:k + 1].contiguous(), iters=8)
        _same_bits(ops.IcpResult(*(f[k:k + 1] for f in a)), one, "image %d alone" % k)


@pytest.mark.parametrize("scale", [True, False])
def test_align_is_the_hand_chained_loop(scale):
    from shapeclipper_amd import ops
    src, dst = ref.unmatched_case()
    src, dst = _dev(np.stack([src, src[::-1]])), _dev(np.stack([dst, dst[::-1]]))
    k = 3
    T = torch.eye(4, dtype=torch.float64, device=DEV).repeat(2, 1, 1)
    s = torch.ones(2, dtype=torch.float64, device=DEV)
    obj = []
    for j in range(k + 1):
        cur = ops.icp_apply(src, T)
        d1, d2, i1, i2 = _search(cur, dst)
        obj.append(ops.icp_objective(d1, d2))
        if j < k:
            T, s = ops.icp_fit(src, dst, i1, i2, scale=scale)
    _same_bits(ops.icp_align(src, dst, iters=k, scale=scale), ops.IcpResult(T, s, cur, d1, d2, i1, i2, torch.stack(obj, dim=1)), "hand-chained")


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(generic):
    from shapeclipper_amd import ops
    src, dst, i1, i2 = (_dev(x) for x in generic)
    T = torch.eye(4, dtype=torch.float64, device=DEV).repeat(3, 1, 1)
    with pytest.raises(TypeError):
        ops.icp_fit(src.double(), dst, i1, i2)
    with pytest.raises(TypeError):
        ops.icp_fit(src, dst, i1.long(), i2)
    with pytest.raises(TypeError):
        ops.icp_apply(src, T.float())
    with pytest.raises(TypeError):
        ops.icp_align(src.half(), dst)
    with pytest.raises(ValueError):
        ops.icp_fit(src, dst, i1[:, :-1].contiguous(), i2)
    with pytest.raises(ValueError):
        ops.icp_fit(src, dst, i2, i1)
    with pytest.raises(ValueError):
        ops.icp_fit(src[..., :2].contiguous(), dst, i1, i2)
    with pytest.raises(ValueError):
        ops.icp_apply(src, T[:, :3].contiguous())
    with pytest.raises(ValueError):
        ops.icp_align(src.view(-1, 3), dst)
    for fn in (lambda: ops.icp_fit(src, dst[:2].contiguous(), i1, i2[:2].contiguous()), lambda: ops.icp_align(src, dst[:2].contiguous()),
               lambda: ops.icp_apply(src, T[:2].contiguous())):
        with pytest.raises(ValueError):                                                         # mismatched B
            fn()
    with pytest.raises(ValueError):
        ops.icp_fit(src, dst.cpu(), i1, i2)
    with pytest.raises(ValueError):
        ops.icp_align(src, dst.cpu())
    with pytest.raises(ValueError):
        ops.icp_apply(src, T.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.icp_align(src.cpu(), dst.cpu())
    with pytest.raises(ValueError, match="contiguous"):
        ops.icp_align(src.transpose(0, 1).contiguous().transpose(0, 1), dst)
    with pytest.raises(ValueError, match="contiguous"):
        ops.icp_fit(src, dst, i1.t().contiguous().t(), i2)
    with pytest.raises(ValueError, match="contiguous"):
        ops.icp_apply(src, T.transpose(1, 2))
    for bad in (0, 101, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="iters"):
            ops.icp_align(src, dst, iters=bad)


def test_raw_c_abi(generic):
    from shapeclipper_amd import _lib, ops
    lib = _lib.load()
    src, dst, i1, i2 = (_dev(x) for x in generic)
    B, N, M = 3, 1000, 1500
    nbytes = int(lib.sc_icp_workspace_bytes(B, N, M))
    assert nbytes == B * 3 * 128 and lib.sc_icp_workspace_bytes(0, N, M) == 0 and lib.sc_icp_workspace_bytes(B, 0, M) == -1
    ws = torch.full((nbytes,), 0xA5, device=DEV, dtype=torch.uint8)                             # contents irrelevant on entry
    T = torch.full((B, 4, 4), -7.0, device=DEV, dtype=torch.float64)
    s = torch.full((B,), -7.0, device=DEV, dtype=torch.float64)
    p, st = _lib.ptr, _lib.stream
    assert lib.sc_icp_fit(p(src), p(dst), p(i1), p(i2), B, N, M, 1, None, None, p(ws), p(T), p(s), st()) == 0
    want, want_s = ops.icp_fit(src, dst, i1, i2)
    assert torch.equal(_bits(T), _bits(want)) and torch.equal(_bits(s), _bits(want_s))
    out = torch.full((B, N, 3), -7.0, device=DEV)
    assert lib.sc_icp_apply(p(src), p(T), B, N, p(out), st()) == 0
    assert torch.equal(_bits(out), _bits(ops.icp_apply(src, want)))
    # n_images <= 0 and refused arguments launch nothing: the outputs keep their fill
    T2, s2, out2 = torch.full_like(T, -7.0), torch.full_like(s, -7.0), torch.full_like(out, -7.0)
    obj = torch.full((B,), -7.0, device=DEV, dtype=torch.float64)
    d1, d2 = torch.rand(B, N, device=DEV), torch.rand(B, M, device=DEV)
    for n_images in (0, -1):
        assert lib.sc_icp_fit(p(src), p(dst), p(i1), p(i2), n_images, N, M, 1, None, None, p(ws), p(T2), p(s2), st()) == 0
        assert lib.sc_icp_apply(p(src), p(T), n_images, N, p(out2), st()) == 0
        assert lib.sc_icp_objective(p(d1), p(d2), n_images, N, M, p(ws), p(obj), 1, st()) == 0
    assert lib.sc_icp_fit(None, p(dst), p(i1), p(i2), B, N, M, 1, None, None, p(ws), p(T2), p(s2), st()) == 1
    assert lib.sc_icp_fit(p(src), p(dst), p(i1), p(i2), B, N, M, 1, None, None, None, p(T2), p(s2), st()) == 1
    assert lib.sc_icp_fit(p(src), p(dst), p(i1), p(i2), B, N, M, 1, p(T), None, p(ws), p(T2), p(s2), st()) == 1      # prev_* go together
    assert lib.sc_icp_fit(p(src), p(dst), p(i1), p(i2), B, 0, M, 1, None, None, p(ws), p(T2), p(s2), st()) == 1
    assert lib.sc_icp_fit(p(src), p(dst), p(i1), p(i2), 65536, N, M, 1, None, None, p(ws), p(T2), p(s2), st()) == 1
    assert lib.sc_icp_apply(p(src), None, B, N, p(out2), st()) == 1
    assert lib.sc_icp_objective(p(d1), None, B, N, M, p(ws), p(obj), 1, st()) == 1
    assert lib.sc_icp_objective(p(d1), p(d2), B, N, M, p(ws), p(obj), 0, st()) == 1
    torch.cuda.synchronize()
    assert bool((T2 == -7).all()) and bool((s2 == -7).all()) and bool((out2 == -7).all()) and bool((obj == -7).all())
    assert lib.sc_icp_objective(p(d1), p(d2), B, N, M, p(ws), p(obj), 1, st()) == 0
    want = d1.double().mean(dim=1) + d2.double().mean(dim=1)
    assert float(((obj - want).abs() / want).max()) < 1e-13


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------------
NEW_FILES = ("chamfer_icp.txt", "cd_cat_icp.txt", "f_score_icp.txt", "icp.txt")
NEW_KEYS = ("dpc_pred_icp", "cd_acc_icp", "cd_comp_icp", "f_score_icp", "icp")


def _opt(extra, output_root):
    from shapeclipper_amd.utils import options
    return options.set(options.parse_arguments(["--yaml=options/pix3d/config.yaml", "--name=pytest_icp", "--output_root=%s" % output_root,
                                                "--arch.enc_pretrained!", "--data.dataset=synthetic", "--eval.num_points=2000", "--tb!", *extra]),
                       verbose=False)


def _runner(o):
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    from shapeclipper_amd.model.runner import Runner
    o.device, o.world_size, o.port = 0, 1, 0
    torch.manual_seed(0)
    r = Runner(o)
    r.load_dataset(o, eval_split="test")
    r.build_networks(o)
    r.graph.eval()
    return r


def _box_grid(o):
    """A level grid whose solid is the box |x| < .3, |y| < .2, |z| < .25 (a Chebyshev-style distance), at get_dense_3D_grid's positions."""
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


def _read_ply_points(data):
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n_v = int([l for l in lines if l.startswith("element vertex")][0].split()[2])
    vdt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    assert end + vdt.itemsize * n_v == len(data)
    return np.frombuffer(data, vdt, n_v, end)


def test_evaluation_writes_the_icp_files_beside_the_raw_ones(tmp_path, monkeypatch):
    from shapeclipper_amd.utils import eval_3D
    o = _opt([], str(tmp_path))
    assert "icp" not in o.eval
    r = _runner(o)
    grid = _box_grid(o)
    monkeypatch.setattr(eval_3D, "HAVE_MESHING", False)
    monkeypatch.setattr(eval_3D, "compute_level_grid", lambda opt, net, z, pts: grid[None].repeat(pts.shape[0], 1, 1, 1))
    n = len(r.test_data)
    net = r.graph.module.sdf_network

    # ---- off: nothing new, in the files or in var ----
    raw_value = r.evaluate(o, ep=0)
    off = _files(o)
    assert not any("icp" in f for f in off), sorted(off)
    assert {"chamfer.txt", "cd_cat.txt", "f_score.txt"} <= set(off)
    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net)
    assert not any(k in var for k in NEW_KEYS)
    raw = (var.cd_acc.clone(), var.cd_comp.clone(), var.f_score.clone(), var.dpc_pred.clone())

    # ---- on ----
    o.eval.icp = True
    o.eval.icp_iters = 12
    assert r.evaluate(o, ep=0) == raw_value                             # the returned value is the raw one
    on = _files(o)
    for f, data in off.items():
        assert on[f] == data, f                                         # every existing output keeps its bytes
    ply = ["dump/%d_pointclouds_comp_icp.ply" % i for i in range(n)]
    assert sorted(set(on) - set(off)) == sorted(list(NEW_FILES) + ply)
    chamfer = [l.split() for l in on["chamfer.txt"].decode().splitlines()]
    chamfer_icp = [l.split() for l in on["chamfer_icp.txt"].decode().splitlines()]
    icp = [l.split() for l in on["icp.txt"].decode().splitlines()]
    assert [int(l[0]) for l in chamfer_icp] == [int(l[0]) for l in icp] == [int(l[0]) for l in chamfer] == list(range(n))
    assert all(len(l) == 3 for l in chamfer_icp) and all(len(l) == 6 and all(len(x.split(".")[1]) == 8 for x in l[1:]) for l in icp)
    for l in icp:
        s, angle, t, first, last = (float(x) for x in l[1:])
        print("icp.txt:", " ".join(l))
        assert last <= first and s > 0 and 0 <= angle <= 180 and t >= 0
    assert any(float(l[5]) < float(l[4]) for l in icp)                  # the registration did something
    assert on["cd_cat_icp.txt"].decode().splitlines()[0] == on["cd_cat.txt"].decode().splitlines()[0]
    assert len(on["cd_cat_icp.txt"].splitlines()) == len(on["cd_cat.txt"].splitlines())
    assert [l.split(":")[0] for l in on["f_score_icp.txt"].decode().splitlines()] == [l.split(":")[0] for l in on["f_score.txt"].decode().splitlines()]
    for i in range(n):
        pts = _read_ply_points(on[ply[i]])
        both = _read_ply_points(on["dump/%d_pointclouds_comp.ply" % i])
        assert len(pts) == len(both) and int((pts["red"] == 255).sum()) == 2000 and int((pts["green"] == 255).sum()) == len(pts) - 2000
        assert np.array_equal(pts[2000:], both[2000:]) and not np.array_equal(pts[:2000], both[:2000])      # same ground truth, moved prediction

    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net)
    assert all(k in var for k in NEW_KEYS) and sorted(var.icp) == ["objective", "s", "transform"]
    assert var.icp["objective"].shape == (1, 13) and var.icp["transform"].shape == (1, 4, 4) and var.dpc_pred_icp.shape == var.dpc_pred.shape
    for a, b in zip(raw, (var.cd_acc, var.cd_comp, var.f_score, var.dpc_pred)):
        assert torch.equal(a, b)                                        # the raw metrics are computed exactly as before
    print("sample 0: cd_acc + cd_comp raw %.6f, after ICP %.6f" % (float(var.cd_acc[0] + var.cd_comp[0]), float(var.cd_acc_icp[0] + var.cd_comp_icp[0])))

    # ---- the sharded evaluation writes the same files from its extra gather ----
    for f in NEW_FILES:
        os.remove(os.path.join(o.output_path, f))
    assert r.evaluate_sharded(o, ep=0) == pytest.approx(raw_value, rel=1e-5)
    sharded = _files(o)
    assert set(sharded) == set(on)
    if sharded["chamfer.txt"] == on["chamfer.txt"]:
        assert sharded["chamfer_icp.txt"] == on["chamfer_icp.txt"] and sharded["icp.txt"] == on["icp.txt"]
        assert sharded["f_score_icp.txt"] == on["f_score_icp.txt"]
    else:
        print("evaluate and evaluate_sharded differ on chamfer.txt: chamfer_icp.txt not compared")
    assert [int(l.split()[0]) for l in sharded["icp.txt"].decode().splitlines()] == list(range(n))

    # ---- an empty mesh: a one-point cloud, the fit keeps the identity, the _icp numbers are the raw ones ----
    empty = torch.ones_like(grid)
    monkeypatch.setattr(eval_3D, "compute_level_grid", lambda opt, net, z, pts: empty[None].repeat(pts.shape[0], 1, 1, 1))
    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net)
    assert bool((var.dpc_pred == var.dpc_pred[:, :1]).all())
    assert torch.equal(var.icp["transform"][0].cpu(), torch.eye(4, dtype=torch.float64)) and float(var.icp["s"][0]) == 1.0
    assert torch.equal(var.cd_acc_icp, var.cd_acc) and torch.equal(var.cd_comp_icp, var.cd_comp) and torch.equal(var.f_score_icp, var.f_score)
    assert torch.equal(var.dpc_pred_icp, var.dpc_pred)

    # ---- vis_only skips it ----
    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net, vis_only=True)
    assert not any(k in var for k in NEW_KEYS)
