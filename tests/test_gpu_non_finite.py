"""Localized non-finite values: a NaN / +-Inf in ONE point, sample, image or ray stays there.

The kernels work on 16-point tiles that straddle two images when n_per_image % 16 != 0, clamp and mask ragged tails and reduce
per-image partial sums, so a poisoned element could leak into its neighbours or be silently dropped.  Each check here derives the
expected poisoned set from the float64 oracle on the same poisoned inputs and runs in both the bf16x3 split form (the default) and
the fp32-MFMA form, for NaN, +Inf and -Inf.  Everything outside the poisoned set must be BIT-identical to the clean run.

Also here: the robust normal loss with NaN normals in the mask (csrc/loss.hip ranks them last, as torch.sort does), reads past the
end of interior slices of NaN-padded buffers, and the fp32 -> bf16 / fp16 conversions of the CLIP tower over all 2^32 inputs."""
import ctypes
import math
from contextlib import contextmanager

import pytest
import torch

pytestmark = pytest.mark.gpu

POISON = [float("nan"), float("inf"), float("-inf")]
SWITCHES = ("SDF_FWD_STREAM", "RGB_FWD_SPLIT", "RGB_BWD_SPLIT", "SDF_VALUE_SPLIT")


@contextmanager
def _form(split):
    """split=True: the default bf16x3 kernels; False: their fp32-MFMA twins.  The switches are restored however the block exits."""
    from shapeclipper_amd import ops
    saved = {k: getattr(ops, k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            setattr(ops, k, split)
        yield
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)


def _bits_equal(a, b):
    """Bit-identical, NaN payloads included."""
    a, b = a.detach().contiguous(), b.detach().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _sdf_case(B, N, seed=0):
    from oracle import reference_ops as R
    cfg = R.Cfg()
    g = torch.Generator().manual_seed(seed)
    W = {k: v + 0.05 * torch.randn(v.shape, generator=g) for k, v in R.init_sdf_weights(cfg, 1).items()}
    z = torch.randn(B, 64, generator=g)
    pts = torch.rand(B * N, 3, generator=g) * 2 - 1
    return cfg, W, z, pts


def _oracle_sdf64(cfg, W, z, pts, B):
    """float64 oracle (sdf [N], grad [N,3], feat [N,64])."""
    from oracle import reference_ops as R
    with R.default_dtype(torch.float64):
        s, f, gr = R.sdf_conditional(cfg, {k: v.double() for k, v in W.items()}, B, pts.double().clone(), z.double(), compute_grad=True)
    return s[:, 0].detach(), gr.detach(), f.detach()


def _hip_sdf(W, pts, n_per_image, z=None, cb=None):
    from shapeclipper_amd import ops, packing
    dev = torch.device("cuda:0")
    pack, cb0 = packing.pack_sdf({k: v.to(dev) for k, v in W.items()}, z.to(dev))
    sdf, grad, feat = ops.sdf_forward(pts.to(dev).contiguous(), pack, cb0 if cb is None else cb, n_per_image, want_grad=True, want_feat=True)
    torch.cuda.synchronize()
    return sdf.cpu(), grad.cpu(), packing.tbl_to_rows(feat, pts.shape[0]).cpu()


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("value", POISON)
@pytest.mark.parametrize("point", [20, 50])        # inside the tile of points 16..31 (images 0 | 1 | 2 at 17, 34) / the last point of the ragged tail
def test_sdf_forward_one_poisoned_point_stays_in_its_row(split, value, point):
    B, N = 3, 17
    cfg, W, z, pts = _sdf_case(B, N)
    bad = pts.clone()
    bad[point, 0] = value
    o_sdf, o_grad, o_feat = _oracle_sdf64(cfg, W, z, bad, B)
    with _form(split):
        clean = _hip_sdf(W, pts, N, z)
        got = _hip_sdf(W, bad, N, z)
    for name, c, x, o in zip(("sdf", "grad", "feat"), clean, got, (o_sdf, o_grad, o_feat)):
        want_bad = ~torch.isfinite(o)
        assert want_bad.view(want_bad.shape[0], -1).any(1).nonzero().flatten().tolist() == [point], name     # the oracle poisons that row alone
        assert torch.equal(~torch.isfinite(x), want_bad), name
        keep = torch.ones(x.shape[0], dtype=torch.bool)
        keep[point] = False
        assert _bits_equal(x[keep], c[keep]), name


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("value", POISON)
def test_sdf_forward_one_poisoned_image_latent_stays_in_its_image(split, value):
    """Image 1's latent poisoned: the kernel and the oracle get the same poisoned z (the kernel through its packed latent biases)."""
    B, N = 3, 17
    cfg, W, z, pts = _sdf_case(B, N, seed=1)
    zb = z.clone()
    zb[1] = value
    o_sdf, o_grad, o_feat = _oracle_sdf64(cfg, W, zb, pts, B)
    with _form(split):
        clean = _hip_sdf(W, pts, N, z)
        got = _hip_sdf(W, pts, N, zb)
    img1 = torch.zeros(B * N, dtype=torch.bool)
    img1[N:2 * N] = True
    for name, c, x, o in zip(("sdf", "grad", "feat"), clean, got, (o_sdf, o_grad, o_feat)):
        rows_bad = (~torch.isfinite(o)).view(B * N, -1).any(1)
        assert torch.equal(rows_bad, img1), name
        assert torch.equal((~torch.isfinite(x)).view(B * N, -1).any(1), img1), name
        assert _bits_equal(x[~img1], c[~img1]), name


def _render_case(B=3, Rr=48, seed=7):
    from oracle import reference_ops as R
    from shapeclipper_amd.utils import options
    opt = options.set(options.parse_arguments(["--yaml=options/pix3d/config.yaml", "--name=pytest", "--output_root=/tmp/sc_pytest"]),
                      verbose=False)
    opt.H, opt.W = 32, 32
    cfg = R.Cfg(H=32, W=32)
    g = torch.Generator().manual_seed(seed)
    trig = lambda t: torch.stack([torch.cos(t), torch.sin(t)], 1)
    az, el = (torch.rand(B, generator=g) * 2 - 1) * math.pi, (torch.rand(B, generator=g) - 0.5) * math.pi / 3
    sd = 0.9 + 0.2 * torch.rand(B, generator=g)
    pose = R.pose_from_trig(cfg, trig(az), trig(el), trig(torch.zeros(B)), sd)
    intr = R.get_intr(cfg, torch.ones(B))
    zs, zr = torch.randn(B, 64, generator=g) * 0.3, torch.randn(B, 64, generator=g) * 0.3
    centre = torch.tensor([y * 32 + x for y in range(6, 26) for x in range(6, 26)])
    ray_idx = torch.stack([centre[torch.randperm(centre.numel(), generator=g)[:Rr]] for _ in range(B)])
    Ws = {k: v + 0.01 * torch.randn(v.shape, generator=g) for k, v in R.init_sdf_weights(cfg, 1).items()}
    Wr = R.init_rgb_weights(cfg, 2)
    return opt, cfg, Ws, Wr, dict(pose=pose, intr=intr, scale_dist=sd, z_sdf=zs, z_rgb=zr), ray_idx


def _hip_render(opt, Ws, Wr, leaves, ray_idx, cot, beta=0.1):
    """One training render + gradients of a cotangent functional: (outputs, leaf grads, weight grads), all on the CPU."""
    from shapeclipper_amd.model.implicit import RGBNetwork, SDFNetwork
    from shapeclipper_amd.model.renderer import Renderer
    dev = torch.device("cuda:0")
    sdf_net, rgb_net = SDFNetwork(opt), RGBNetwork(opt)
    sdf_net.load_state_dict(Ws)
    rgb_net.load_state_dict(Wr)
    r = Renderer(opt, sdf_net, rgb_net).to(dev)
    with torch.no_grad():
        r.density.beta.fill_(beta)
    lv = {k: v.detach().to(dev).requires_grad_(True) for k, v in leaves.items()}
    torch.manual_seed(1234)
    out = r(opt, lv["pose"], lv["intr"], lv["scale_dist"], lv["z_sdf"], lv["z_rgb"], ray_idx=ray_idx.to(dev), training=True)
    rgb, mask, mask_hard, depth, normal, eik = out
    cd = {k: v.to(dev) for k, v in cot.items()}
    L = (rgb * cd["rgb"]).sum() + (mask * cd["mask"]).sum() + (depth * cd["depth"]).sum() + (normal * cd["normal"]).sum() + (eik * cd["eik"]).sum()
    params = dict(r.named_parameters())
    g = torch.autograd.grad(L, list(lv.values()) + list(params.values()), allow_unused=True)
    torch.cuda.synchronize()
    outs = dict(rgb=rgb, mask=mask, mask_hard=mask_hard, depth=depth, normal=normal, eik=eik)
    return ({k: v.detach().cpu() for k, v in outs.items()}, {k: x.cpu() for k, x in zip(lv, g[:len(lv)])},
            {k: (x.cpu() if x is not None else None) for k, x in zip(params, g[len(lv):])})


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("value", POISON)
def test_training_render_one_poisoned_pose_stays_in_its_image(split, value):
    """Image 1's camera translation poisoned: its outputs are non-finite, the other images' outputs and leaf gradients are bit-identical
    to the clean run, and the shared weight gradients are non-finite (one exception, below).  The float64 oracle agrees on the set."""
    from oracle import reference_ops as R
    B, Rr = 3, 48
    opt, cfg, Ws, Wr, leaves, ray_idx = _render_case(B, Rr)
    bad = dict(leaves)
    bad["pose"] = leaves["pose"].clone()
    bad["pose"][1, 2, 3] = value
    g = torch.Generator().manual_seed(3)
    cot = dict(rgb=torch.randn(B, Rr, 3, generator=g), mask=torch.randn(B, Rr, 1, generator=g), depth=torch.randn(B, Rr, 1, generator=g),
               normal=torch.randn(B, Rr, 3, generator=g), eik=torch.randn(2 * B * Rr, generator=g))
    # float64 oracle on the poisoned inputs: which images' outputs are non-finite
    torch.manual_seed(1234)
    t_rand, eik_idx, eik_pts = R.draw_render_randoms(B * Rr, 64, True)
    with R.default_dtype(torch.float64):
        o = R.render(cfg, {k: v.double() for k, v in Ws.items()}, {k: v.double() for k, v in Wr.items()}, torch.tensor(0.1),
                     bad["pose"].double(), bad["intr"].double(), bad["scale_dist"].double(), bad["z_sdf"].double(), bad["z_rgb"].double(),
                     ray_idx, True, t_rand.double(), eik_idx, eik_pts.double())
    for k in ("rgb", "mask", "depth", "normal"):
        img_bad = (~torch.isfinite(o[k])).view(B, -1).all(1)
        assert img_bad.tolist() == [False, True, False], k
    with _form(split):
        c_out, c_lv, _ = _hip_render(opt, Ws, Wr, leaves, ray_idx, cot)
        p_out, p_lv, p_w = _hip_render(opt, Ws, Wr, bad, ray_idx, cot)
    others = [0, 2]
    for k in ("rgb", "mask", "depth", "normal"):
        assert (~torch.isfinite(p_out[k][1])).all(), k
        assert _bits_equal(p_out[k][others], c_out[k][others]), k
    assert not bool(p_out["mask_hard"][1].any())                    # NaN > 0.5 is False, as in the oracle
    assert _bits_equal(p_out["mask_hard"][others], c_out["mask_hard"][others])
    # eikonal points: [image][random points R | points on the rays R]; the rays of image 1 start at its poisoned camera
    pe, ce = p_out["eik"].view(B, 2 * Rr), c_out["eik"].view(B, 2 * Rr)
    assert (~torch.isfinite(pe[1, Rr:])).all() and _bits_equal(pe[others], ce[others]) and _bits_equal(pe[1, :Rr], ce[1, :Rr])
    for k in ("z_sdf", "z_rgb", "scale_dist", "pose", "intr"):
        assert torch.isfinite(p_lv[k][others]).all(), k
        assert _bits_equal(p_lv[k][others], c_lv[k][others]), k
    # Finding: the RGB network's ReLUs map a NaN pre-activation to 0 (v_max_f32); torch's relu keeps the NaN.  Image 1's hidden RGB
    # activations are therefore finite (zero after the first layer), its ReLU masks zero the matching gradient rows, and some RGB bias
    # gradients stay finite: lin0.bias in the split form, lin0.bias, lin1.bias and lin2.bias in the fp32 form -- exactly those; every
    # other shared gradient (the SDF network's, beta's, the other RGB tensors) is non-finite.
    finite_ok = {"rgb_network.lin0.bias"} if split else {"rgb_network.lin0.bias", "rgb_network.lin1.bias", "rgb_network.lin2.bias"}
    finite = {k for k, gw in p_w.items() if gw is not None and bool(torch.isfinite(gw).all())}
    print("finite shared gradients (split=%s):" % split, sorted(finite))
    for k, gw in p_w.items():
        if gw is not None:
            assert torch.isfinite(gw).all() == (k in finite_ok), "weight gradient finite: %s (expected %s)" % (k, k in finite_ok)


# ---------------------------------------------------------------------------------------------------------------------------------
# robust normal loss: NaN normals inside the mask
# ---------------------------------------------------------------------------------------------------------------------------------
def _loss_inputs(B=2, Rr=100, seed=5):
    g = torch.Generator().manual_seed(seed)
    rgb, tgt = torch.rand(B, Rr, 3, generator=g), torch.rand(B, Rr, 3, generator=g)
    pm, tm = torch.rand(B, Rr, 1, generator=g), (torch.rand(B, Rr, 1, generator=g) > 0.4).float()
    npred = torch.nn.functional.normalize(torch.randn(B, Rr, 3, generator=g), dim=-1)
    ngt = torch.nn.functional.normalize(torch.randn(B, Rr, 3, generator=g), dim=-1)
    return rgb, tgt, pm, tm, npred, ngt


def _fused_loss(rgb, tgt, pm, tm, npred, ngt, tol):
    from shapeclipper_amd import ops
    dev = torch.device("cuda:0")
    d = lambda t: t.to(dev)
    out, grads = ops.loss_fused_forward(d(rgb), d(tgt), d(pm), d(tm), d(npred), d(ngt), None, 5.0, 0.0, 1 - tol, want_target_grad=True)
    torch.cuda.synchronize()
    return out.cpu(), [x.cpu() for x in grads if x is not None]


@pytest.mark.parametrize("tol", [0.2, 0.0])
def test_normal_loss_with_nan_normals_in_the_mask_matches_torch(tol):
    """k masked rays with a NaN normal.  torch.sort ranks NaN last, so the loss is finite while k <= n - n_keep and NaN beyond; the
    kernel used to drop the NaN rays from the candidates and then read a threshold it had never written (a finite value that changed
    from run to run).  Two runs must also be bit-identical, gradients included."""
    from oracle import reference_ops as R
    rgb, tgt, pm, tm, npred, ngt = _loss_inputs()
    mask = (tm > 0.5) & (pm > 0.5)
    n = int(mask.sum())
    n_keep = int(n * (1 - tol))
    masked = mask.view(-1).nonzero().flatten()
    order = masked[torch.randperm(n, generator=torch.Generator().manual_seed(1))]
    for k in sorted({1, n - n_keep, n - n_keep + 1}):
        bad = npred.clone()
        bad.view(-1, 3)[order[:k]] = float("nan")
        ref = float(R.normal_loss(R.Cfg(), bad, ngt, mask, tolerance=tol))
        out, grads = _fused_loss(rgb, tgt, pm, tm, bad, ngt, tol)
        out2, grads2 = _fused_loss(rgb, tgt, pm, tm, bad, ngt, tol)
        got = float(out[2])
        print("tol %.1f n %d n_keep %d k %d: kernel %r torch %r" % (tol, n, n_keep, k, got, ref))
        assert math.isnan(got) == math.isnan(ref), (k, got, ref)
        assert math.isnan(ref) == (k > n - n_keep)
        if not math.isnan(ref):
            assert abs(got - ref) < 2e-5 * max(1.0, abs(ref)), (k, got, ref)
        assert _bits_equal(out, out2), k
        for a, b in zip(grads, grads2):
            assert _bits_equal(a, b), k


# ---------------------------------------------------------------------------------------------------------------------------------
# unwritten outputs and reads past the end: interior slices of NaN-padded buffers, NaN-poisoned blocks from the caching allocator
# ---------------------------------------------------------------------------------------------------------------------------------
def _padded(t, pad=4096):
    """t's values as an interior slice of a NaN-filled buffer (pad elements of NaN on both sides)."""
    flat = torch.full((t.numel() + 2 * pad,), float("nan"), device=t.device, dtype=t.dtype)
    flat[pad:pad + t.numel()] = t.reshape(-1)
    return flat[pad:pad + t.numel()].view(t.shape)


def _poison_allocator(n_floats):
    """Allocate and free a NaN tensor: the caching allocator hands the same block to the next allocation of that size."""
    x = torch.full((n_floats,), float("nan"), device="cuda:0")
    del x


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("B,N", [(1, 1), (2, 17), (3, 1371)])
def test_sdf_forward_ignores_nan_padding_and_poisoned_blocks(split, B, N):
    from shapeclipper_amd import ops, packing
    cfg, W, z, pts = _sdf_case(B, N, seed=B + N)
    dev = torch.device("cuda:0")
    pack, cb = packing.pack_sdf({k: v.to(dev) for k, v in W.items()}, z.to(dev))
    p = pts.to(dev)
    with _form(split):
        ref = ops.sdf_forward(p, pack, cb, N)
        ref = [ref[0].clone(), ref[1].clone(), packing.tbl_to_rows(ref[2], B * N).clone()]
        args = (_padded(p), _padded(pack), _padded(cb))        # the padded inputs first: the poisoned blocks go to the op's outputs
        for n in (B * N, B * N * 3, packing.n_tiles(B * N) * 1024):
            _poison_allocator(n)
        got = ops.sdf_forward(*args, N)
        got = [got[0], got[1], packing.tbl_to_rows(got[2], B * N)]
        torch.cuda.synchronize()
    for name, a, b in zip(("sdf", "grad", "feat"), got, ref):
        assert torch.isfinite(a).all(), name
        assert _bits_equal(a, b), name


@pytest.mark.parametrize("B,Rr", [(1, 5), (3, 37)])
def test_fused_loss_ignores_nan_padding_and_poisoned_blocks(B, Rr):
    from shapeclipper_amd import ops
    dev = torch.device("cuda:0")
    ins = [t.to(dev) for t in _loss_inputs(B, Rr, seed=B * Rr)]
    ins[2], ins[3] = 0.5 + 0.5 * ins[2], torch.ones_like(ins[3])         # every ray in the mask: the normal loss is finite
    eik = torch.rand(B, 2 * Rr, device=dev) + 0.5
    ref_out, ref_g = ops.loss_fused_forward(*ins, eik, 5.0, 0.3, 0.8, want_target_grad=True)
    ref_out, ref_g = ref_out.clone(), [g.clone() for g in ref_g]
    args = [_padded(t) for t in ins] + [_padded(eik)]          # the padded inputs first: the poisoned blocks go to the op's outputs
    for n in (B * Rr, B * Rr * 3, B * 2 * Rr, B * Rr + 4 * B):
        _poison_allocator(n)
    out, g = ops.loss_fused_forward(*args, 5.0, 0.3, 0.8, want_target_grad=True)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and _bits_equal(out, ref_out)
    for a, b in zip(g, ref_g):
        assert torch.isfinite(a).all() and _bits_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 -> 16-bit conversions of the CLIP tower (csrc/clip_vit.hip f2bf / cvt16, gemm8p.hpp pack2)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_f32_to_16bit_conversion_all_bit_patterns(kind):
    """All 2^32 fp32 bit patterns, 2^28 at a time, against torch's conversion: bit-identical for every non-NaN input, NaN for NaN.
    The bf16 rounding used to carry NaNs with a large payload into +-Inf or -0 (0x7F800001 -> 0x7F80, 0x7FFF8000 -> 0x8000)."""
    from shapeclipper_amd import _lib
    lib = _lib.load()
    fn, td = (lib.sc_f32_to_bf16, torch.bfloat16) if kind == "bf16" else (lib.sc_f32_to_f16, torch.float16)
    exp_mask = 0x7F80 if kind == "bf16" else 0x7C00
    dev = torch.device("cuda:0")
    chunk = 1 << 28
    base = torch.arange(chunk, device=dev, dtype=torch.int64)
    y = torch.empty(chunk, device=dev, dtype=torch.int16)
    n_bad = 0
    for c in range(1 << 4):
        u = (base + (c * chunk - (1 << 31))).to(torch.int32)       # signed view of the patterns c * 2^28 ...
        x = u.view(torch.float32)
        assert fn(_lib.ptr(x), _lib.ptr(y), ctypes.c_longlong(chunk), _lib.stream()) == 0
        want = x.to(td).view(torch.int16)
        nan = torch.isnan(x)
        y_nan = (y.to(torch.int32) & 0x7FFF) > exp_mask
        n_bad += int((~nan & (y != want)).sum()) + int((nan & ~y_nan).sum())
        del u, x, want, nan, y_nan
    torch.cuda.synchronize()
    assert n_bad == 0, n_bad
    one = torch.tensor([0x7F800001, 0x7FFF8000, -1], dtype=torch.int32, device=dev).view(torch.float32)     # -1: 0xFFFFFFFF
    y3 = torch.empty(3, device=dev, dtype=torch.int16)
    assert fn(_lib.ptr(one), _lib.ptr(y3), ctypes.c_longlong(3), _lib.stream()) == 0
    assert torch.isnan(y3.view(td).float()).all()


@pytest.mark.parametrize("M,N,K", [(2049, 256, 64), (2049, 6144, 64), (4100, 3328, 192)])
@pytest.mark.parametrize("epi", [2, 3])
def test_gemm_bf16_epilogue_non_finite_rows(epi, M, N, K):
    """NaN / +-Inf planted in rows of A and a NaN in one bias column: the bf16 output of epilogues 2 (quick_gelu) and 3 is non-finite
    exactly where float64 is."""
    from shapeclipper_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    A = (torch.randn(M, K, device=dev, generator=g) * 0.5).to(torch.bfloat16)
    W = (torch.randn(N, K, device=dev, generator=g) * 0.1).to(torch.bfloat16)
    bias = torch.randn(N, device=dev, generator=g)
    rows = [0, 17, M - 1]
    for r, v in zip(rows, POISON):
        A[r, (r * 7) % K] = v
    # a NaN with a full payload in the bias: the epilogue's fp32 -> bf16 rounding used to carry it into -0 (0x7FFFFFFF -> 0x8000)
    col = N // 2 + 3
    bias.view(torch.int32)[col] = 0x7FFFFFFF
    out = torch.zeros(M, N, device=dev, dtype=torch.bfloat16)
    rc = lib.sc_gemm_bf16(ctypes.c_int(epi), _lib.ptr(A), _lib.ptr(W), _lib.ptr(bias), _lib.ptr(out), ctypes.c_int(M), ctypes.c_int(N),
                          ctypes.c_int(K), _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    ref = A.double() @ W.double().t() + bias.double()
    if epi == 2:
        ref = ref * torch.sigmoid(1.702 * ref)
    want = ~torch.isfinite(ref)
    cols = torch.ones(N, dtype=torch.bool, device=dev)
    cols[col] = False
    assert want[:, cols].any(1).nonzero().flatten().tolist() == rows and bool(want[:, col].all())
    assert torch.equal(~torch.isfinite(out.float()), want)
    ok = ~want
    assert float(((out.double() - ref)[ok]).abs().max()) < 1e-2 * float(ref[ok].abs().max())


# ---------------------------------------------------------------------------------------------------------------------------------
# kernel-level backward: one poisoned point of the SDF backward, one poisoned sample of the RGB compositing
# ---------------------------------------------------------------------------------------------------------------------------------
def _sdf_grads(W, z, pts, N, c):
    """Every gradient of <sdf, c1> + <d sdf/dx, c2> + <feat, c3> through SdfFunction (the fused backward when N % 16 == 0)."""
    from shapeclipper_amd import packing
    from shapeclipper_amd.functional import SdfFunction
    dev = torch.device("cuda:0")
    Wd = {k: v.to(dev).requires_grad_(True) for k, v in W.items()}
    zd, pd = z.to(dev).requires_grad_(True), pts.to(dev).requires_grad_(True)
    pack, cb = packing.pack_sdf(Wd, zd)
    sdf, grad, feat = SdfFunction.apply(pd, pack, cb, N, True, True, True, True)
    L = (sdf * c[0].to(dev)).sum() + (grad * c[1].to(dev)).sum() + (packing.tbl_to_rows(feat, pts.shape[0]) * c[2].to(dev)).sum()
    gs = torch.autograd.grad(L, list(Wd.values()) + [zd, pd])
    torch.cuda.synchronize()
    return dict(zip(list(Wd) + ["z", "points"], [x.cpu() for x in gs]))


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("value", POISON)
@pytest.mark.parametrize("N,point", [(17, 20), (32, 40)])      # a tile straddling images 0 | 1 (unfused backward); the fused backward
def test_sdf_backward_one_poisoned_point(split, value, N, point):
    """Finite cotangents, one point poisoned: every shared weight gradient is non-finite, the other images' latent gradients and the
    other points' gradients are bit-identical to the clean run, and the poisoned image's latent gradient is non-finite.  (The last
    layer's bias is the exception by the chain rule: d L / d lin5.bias = sum of the cotangents, which do not depend on the points.)"""
    B = 3
    cfg, W, z, pts = _sdf_case(B, N, seed=N)
    g = torch.Generator().manual_seed(5)
    c = (torch.randn(B * N, generator=g), torch.randn(B * N, 3, generator=g), torch.randn(B * N, 64, generator=g) * 0.1)
    bad = pts.clone()
    bad[point, 1] = value
    with _form(split):
        clean = _sdf_grads(W, z, pts, N, c)
        got = _sdf_grads(W, z, bad, N, c)
    img = point // N
    others = [b for b in range(B) if b != img]
    assert _bits_equal(got["lin5.bias"], clean["lin5.bias"])
    for k in W:
        if k != "lin5.bias":
            assert not torch.isfinite(got[k]).all(), "weight gradient silently finite: " + k
    assert not torch.isfinite(got["z"][img]).all()
    assert _bits_equal(got["z"][others], clean["z"][others])
    keep = torch.ones(B * N, dtype=torch.bool)
    keep[point] = False
    assert _bits_equal(got["points"][keep], clean["points"][keep])


def _rgb_inputs(n_images, rpi, seed):
    from oracle import reference_ops as R
    from shapeclipper_amd import ops, packing
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(seed)
    cfg = R.Cfg()
    Ws, Wr = R.init_sdf_weights(cfg, 1), R.init_rgb_weights(cfg, 2)
    zs, zr = torch.randn(n_images, 64, generator=g) * 0.3, torch.randn(n_images, 64, generator=g) * 0.3
    n_rays = n_images * rpi
    pts = (torch.rand(n_rays * 64, 3, generator=g) * 1.6 - 0.8).to(dev)
    z = torch.sort(torch.rand(n_rays, 64, generator=g) * 2 + 4, dim=1).values.to(dev)
    dfac = (torch.rand(n_rays, generator=g) * 0.2 + 0.9).to(dev)
    sdf_pack, cb = packing.pack_sdf({k: v.to(dev) for k, v in Ws.items()}, zs.to(dev))
    sdf, grad, feat = ops.sdf_forward(pts, sdf_pack, cb, rpi * 64)
    v_pack, dbias = packing.pack_rgb({k: v.to(dev) for k, v in Wr.items()}, zr.to(dev))
    G = dict(G_rgb=torch.randn(n_rays, 3, generator=g).to(dev), G_mask=torch.randn(n_rays, generator=g).to(dev),
             G_depth=torch.randn(n_rays, generator=g).to(dev), G_normal=torch.randn(n_rays, 3, generator=g).to(dev))
    return dict(points=pts, z_vals=z, depth_fac=dfac, sdf=sdf, grad=grad, feat=feat, v_pack=v_pack, dbias=dbias,
                beta=torch.tensor([0.1], device=dev)), G


def _rgb_run(x, G, rpi):
    """Forward (parking the activations, as the training step does) + fused backward -> (outputs, gradients)."""
    from shapeclipper_amd import ops
    args = (x["points"], x["z_vals"], x["depth_fac"], x["sdf"], x["grad"], x["feat"], x["v_pack"], x["dbias"], x["beta"])
    o = ops.rgb_composite_forward(*args, rpi, True, 1e-4, 1.0, 1.0, keep_rgb_flat=True, keep_rr=True)
    g = ops.rgb_composite_backward(*args, o["rgb_flat"], rpi, True, 1e-4, 1.0, 1.0, G["G_rgb"], G["G_mask"], G["G_depth"], G["G_normal"],
                                   rr=o["rr"])
    torch.cuda.synchronize()
    return {k: o[k].clone() for k in ("rgb", "mask", "mask_hard", "depth", "normal")}, {k: v.clone() for k, v in g.items()}


@pytest.mark.parametrize("split", [True, False])
def test_rgb_composite_one_poisoned_sample(split):
    """One sample's sdf NaN, finite cotangents: exactly that ray's rgb, mask, depth and normal are non-finite (its mask_hard is the
    oracle's: NaN > 0.5 is False), every other ray's outputs and every other ray's point / sdf / d sdf/dx gradients are bit-identical to the
    clean run, the other image's latent-bias gradient is bit-identical and the RGB weight and beta gradients are non-finite.
    (+-Inf sdf is a legitimate density, 0 or 1/beta.  A poisoned FEATURE is not checked here: the RGB network's ReLUs map NaN to 0,
    see test_training_render_one_poisoned_pose_stays_in_its_image.)"""
    n_images, rpi = 2, 37
    x, G = _rgb_inputs(n_images, rpi, seed=3)
    ray, sample = 40, 17                         # image 1
    bad = dict(x)
    bad["sdf"] = x["sdf"].clone()
    bad["sdf"][ray * 64 + sample] = float("nan")
    with _form(split):
        c_o, c_g = _rgb_run(x, G, rpi)
        p_o, p_g = _rgb_run(bad, G, rpi)
    n_rays = n_images * rpi
    other = torch.ones(n_rays, dtype=torch.bool, device=c_o["rgb"].device)
    other[ray] = False
    for k in ("rgb", "mask", "depth", "normal"):
        assert (~torch.isfinite(p_o[k][ray])).all(), k
        assert _bits_equal(p_o[k][other], c_o[k][other]), k
    # the oracle's mask_hard = (acc > 0.5): False for a NaN accumulation, the clean value for a finite one
    assert float(p_o["mask_hard"][ray]) == 0.0
    assert _bits_equal(p_o["mask_hard"][other], c_o["mask_hard"][other])
    pts_other = other.repeat_interleave(64)
    for k in ("points", "sdf", "grad"):
        assert _bits_equal(p_g[k][pts_other], c_g[k][pts_other]), k
    assert _bits_equal(p_g["dbias"][0], c_g["dbias"][0])
    assert not torch.isfinite(p_g["v_pack"]).all() and not torch.isfinite(p_g["beta"]).all()


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("n_images,rpi", [(1, 5), (3, 37)])
def test_rgb_composite_ignores_nan_padding_and_poisoned_blocks(split, n_images, rpi):
    """rgb_composite_forward / backward on interior slices of NaN-padded inputs, with NaN blocks waiting in the caching allocator for
    their outputs: finite and bit-identical to the unpadded run."""
    x, G = _rgb_inputs(n_images, rpi, seed=n_images + rpi)
    with _form(split):
        ref_o, ref_g = _rgb_run(x, G, rpi)
        xp = {k: _padded(v) for k, v in x.items()}
        Gp = {k: _padded(v) for k, v in G.items()}
        P = n_images * rpi * 64
        for n in (n_images * rpi, n_images * rpi * 3, P, P * 3, P * 16, 3 * n_images * rpi * 4 * 1024):
            _poison_allocator(n)
        got_o, got_g = _rgb_run(xp, Gp, rpi)
    for k in ref_o:
        assert torch.isfinite(got_o[k]).all() and _bits_equal(got_o[k], ref_o[k]), k
    for k in ref_g:
        assert torch.isfinite(got_g[k]).all() and _bits_equal(got_g[k], ref_g[k]), k


# ---------------------------------------------------------------------------------------------------------------------------------
# the SDF backward (fused and non-fused) and ray sampling on NaN-padded inputs, NaN blocks waiting for their outputs and scratch
# ---------------------------------------------------------------------------------------------------------------------------------
def _poison_scratch():
    """NaN into every cached scratch buffer of ops -- ops._SCRATCH holds them all: forward scratch, parked second-order terms, partial
    images of the row sums and of tbl_sum, and whatever BatchNorm / convolution workspaces earlier tests of the process left there:
    each must be written before it is read."""
    from shapeclipper_amd import ops
    for v in ops._SCRATCH.values():
        v.fill_(float("nan"))


def _sdf_bwd_inputs(B, N, seed):
    from shapeclipper_amd import ops, packing
    cfg, W, z, pts = _sdf_case(B, N, seed=seed)
    dev = torch.device("cuda:0")
    pack, cb = packing.pack_sdf({k: v.to(dev) for k, v in W.items()}, z.to(dev))
    p = pts.to(dev)
    _, _, _, sa, sp = ops.sdf_forward(p, pack, cb, N, stash=True)
    g = torch.Generator().manual_seed(seed + 1)
    n = B * N
    gs, gg = torch.randn(n, generator=g).to(dev), torch.randn(n, 3, generator=g).to(dev)
    gf = packing.rows_to_tbl(torch.randn(n, 64, generator=g) * 0.1).to(dev)
    return dict(points=p, w_pack=pack, stash_a=sa, stash_p=sp, g_sdf=gs, g_grad=gg, g_feat=gf)


def _sdf_bwd_call(x, B, N, fused):
    from shapeclipper_amd import ops
    a = (x["points"], x["w_pack"], N, B, True, x["stash_a"], x["stash_p"], x["g_sdf"], x["g_grad"], x["g_feat"])
    out = ops.sdf_backward_fused(*a) if fused else ops.sdf_backward(*a, fused=False)
    torch.cuda.synchronize()
    return [t.clone() for t in out]


@pytest.mark.parametrize("fused,B,N", [(True, 1, 16), (True, 3, 1040), (False, 3, 17), (False, 3, 74), (False, 1, 1000)])
def test_sdf_backward_ignores_nan_padding_and_poisoned_blocks(fused, B, N):
    """sdf_backward_fused (stash, upstream gradients, points, pack as interior slices of NaN-padded buffers) and the non-fused
    sdf_backward at n_per_image % 16 != 0 (at most 1024 points: one tbl_sum block, so its float atomics add in a fixed order), whose hand-off tensors ga / gp / r0 are whole-tile torch.empty blocks: their padding lanes
    (points past n) come from the caching allocator NaN-filled here, and sc_wgrad / tbl_sum must never sum them."""
    from shapeclipper_amd import _lib, ops, packing
    x = _sdf_bwd_inputs(B, N, seed=B * 100 + N)
    ref = _sdf_bwd_call(x, B, N, fused)
    xp = {k: _padded(v) for k, v in x.items()}
    n, T = B * N, packing.n_tiles(B * N) * 1024
    lib = _lib.load()
    if fused:
        parts, stride = int(lib.sc_sdf_backward_fused_parts(ctypes.c_int(n))), int(lib.sc_sdf_backward_fused_partial_floats(ctypes.c_int(B)))
        sizes = (n * 3, parts * stride, stride, B * 5 * 64)
    else:
        assert int(lib.sc_tbl_sum_blocks(ctypes.c_int(n))) == 1      # one block: its float atomics add in a fixed order (bit-equal runs)
        sizes = (5 * T, 4 * T, T, n * 3, ops.WGRAD_PARTS * packing.SDF_PACK_FLOATS, packing.SDF_PACK_FLOATS, 5 * B * 64, 2 * 64,
                 5 * B * 64)
    _poison_scratch()
    for s in sizes:
        _poison_allocator(s)
    got = _sdf_bwd_call(xp, B, N, fused)
    for name, a, b in zip(("points", "w_pack", "cbias"), got, ref):
        assert torch.isfinite(a).all(), name
        assert _bits_equal(a, b), name


def _ray_inputs(B, R, training, seed):
    g = torch.Generator().manual_seed(seed)
    dev = torch.device("cuda:0")
    n = B * R
    x = dict(cam_loc=torch.randn(n, 3, generator=g), ray_dirs=torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1),
             scale_dist=0.8 + 0.4 * torch.rand(B, generator=g), eik_uniform=torch.rand(n, 3, generator=g) * 2 - 1,
             g_points=torch.randn(n * 64, 3, generator=g), g_z=torch.randn(n, 64, generator=g), g_eik=torch.randn(B, 2 * R, 3, generator=g))
    if training:
        x["u"] = torch.rand(n, 64, generator=g)
    x = {k: v.to(dev) for k, v in x.items()}
    x["eik_idx"] = torch.randint(64, (n,), generator=g).to(dev)
    return x


def _ray_run(x, B, R, eik):
    """forward + backward, plain or with the eikonal points -> dict of every output."""
    from shapeclipper_amd import ops
    u = x.get("u")
    if eik:
        z, p, e = ops.ray_sample_forward_eik(x["cam_loc"], x["ray_dirs"], x["scale_dist"], u, x["eik_idx"], x["eik_uniform"], R, 5.0)
        go, gd, gsd = ops.ray_sample_backward_eik(x["ray_dirs"], z, x["g_points"], x["g_z"], x["eik_idx"], x["g_eik"], R, B, 5.0)
        out = dict(eik=e)
    else:
        z, p = ops.ray_sample_forward(x["cam_loc"], x["ray_dirs"], x["scale_dist"], u, R, 5.0)
        go, gd, gsd = ops.ray_sample_backward(x["ray_dirs"], z, x["g_points"], x["g_z"], R, B, 5.0)
        out = {}
    torch.cuda.synchronize()
    out.update(z=z, points=p, g_cam_loc=go, g_ray_dirs=gd, g_scale_dist=gsd)
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("eik", [True, False])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B,R", [(1, 1), (3, 37)])
def test_ray_sample_ignores_nan_padding_and_poisoned_blocks(B, R, training, eik):
    x = _ray_inputs(B, R, training, seed=B * R + training)
    ref = _ray_run(x, B, R, eik)
    xp = {k: (_padded(v) if v.is_floating_point() else v) for k, v in x.items()}
    n = B * R
    for s in (n * 64, n * 64 * 3, B * 2 * R * 3, n * 3, n):
        _poison_allocator(s)
    got = _ray_run(xp, B, R, eik)
    for k in ref:
        assert torch.isfinite(got[k]).all() and _bits_equal(got[k], ref[k]), k


@pytest.mark.parametrize("eik", [True, False])
@pytest.mark.parametrize("training", [True, False])
def test_ray_sample_one_poisoned_direction_stays_in_its_ray(training, eik):
    """Ray 40 (image 1) gets a NaN direction.  Only its points (and its near-surface eikonal point) and its image's g_scale_dist may
    become non-finite -- they must -- and everything else is bit-identical to the clean run."""
    B, R, ray = 3, 37, 40
    x = _ray_inputs(B, R, training, seed=11 + training)
    clean = _ray_run(x, B, R, eik)
    bad = dict(x)
    bad["ray_dirs"] = x["ray_dirs"].clone()
    bad["ray_dirs"][ray, 1] = float("nan")
    got = _ray_run(bad, B, R, eik)
    n = B * R
    may = {k: torch.zeros_like(v, dtype=torch.bool) for k, v in clean.items()}
    may["points"].view(n, 64, 3)[ray] = True
    may["g_scale_dist"][ray // R] = True
    if eik:
        may["eik"][ray // R, R + ray % R] = True
    for k in clean:
        nf = ~torch.isfinite(got[k])
        assert not (nf & ~may[k]).any(), k
        assert _bits_equal(got[k][~may[k]], clean[k][~may[k]]), k
    assert (~torch.isfinite(got["points"].view(n, 64, 3)[ray])).any() and not torch.isfinite(got["g_scale_dist"][ray // R])
    if eik:
        assert not torch.isfinite(got["eik"][ray // R, R + ray % R]).all()
